"""Model compiler: known answers from the reference's own constants."""
import os

import numpy as np
import pytest

from conftest import ROOT

from locomanipulationrl_amd.model.robot_model import closure_g, LIMB_STRIDE, HUB_FLOATS

CLASS_DEFAULT_Q = [-1.2, 1.2, 1.2, -1.2, -1.22, -1.92, 1.92, 1.22, 1.92, 1.22, -1.22, -1.92]
TASK_Q = [-1.57, 1.57, 1.57, -1.57, -1.04, -2.09, 2.09, 1.04, 2.09, 1.04, -1.04, -2.09]


def test_total_mass(robot_model, vertical_model):
    assert abs(robot_model.total_mass - 2.2559) < 1e-4
    assert abs(vertical_model.total_mass - 2.2566) < 1e-4


def test_fk_known_answer(robot_model):
    # quadruped_pose_control.py:127-130 default_base_tip_positions at robot/quadruped_robot.py:45-52 pose
    expect = np.array([[-0.0937, 0.1223, -0.1774], [0.0937, 0.1408, -0.1773],
                       [-0.0937, -0.1408, -0.1773], [0.0937, -0.1223, -0.1774]])
    tips = robot_model.tip_positions(CLASS_DEFAULT_Q)
    assert np.abs(tips - expect).max() < 1e-4
    # with the reference's rounded passive angles (+-0.953) the same answer comes out
    qt = np.array(CLASS_DEFAULT_Q + [0.953, -0.953] * 4)
    assert np.abs(robot_model.tip_positions(CLASS_DEFAULT_Q, tree_angles=qt) - expect).max() < 1e-4


def test_task_pose_tips(robot_model):
    tips = robot_model.tip_positions(TASK_Q)
    assert np.abs(tips[0] - [-0.1186, 0.1189, -0.1292]).max() < 5e-4       # SURVEY A.4 (rounded passives there)
    assert abs(tips[:, 2].mean() + 0.129) < 5e-4                            # -> 0.011 m above ground at base z 0.14


def test_vertical_pose(vertical_model):
    q = [0, 0, 0, 0] + [0.35, -0.35] * 4
    tips = vertical_model.tip_positions(q)
    assert np.abs(tips[0] - [-0.079, -0.009, -0.3186]).max() < 5e-4


def test_closure_function_values():
    # passive angles the reference ships: 0.953 at D=0.70, 1.37(26) at D=1.05, 0.95 at D=0.70 (vertical)
    g, g1, g2 = closure_g(np.array([0.70, 1.05]))
    assert abs(g[0] - 0.953) < 1e-3 and abs(g[1] - 1.3726) < 1e-4
    eps = 1e-6
    gp, _, _ = closure_g(0.9 + eps); gm, _, _ = closure_g(0.9 - eps)
    _, d1, d2 = closure_g(0.9)
    assert abs((gp - gm) / (2 * eps) - d1) < 1e-8
    _, d1p, _ = closure_g(0.9 + eps); _, d1m, _ = closure_g(0.9 - eps)
    assert abs((d1p - d1m) / (2 * eps) - d2) < 1e-7


def _urdf_from_golden(robot, dest):
    """Write <dest>/<robot>.urdf from tests/golden/urdf_<robot>.npz: the reference URDF's link and joint tables (tools/extract_reference_fixtures.py)
    with only the elements model/urdf.py reads, so that parse_urdf / compile_urdf see the same numbers as on the original file."""
    from xml.sax.saxutils import quoteattr
    from conftest import GOLDEN
    t = np.load(os.path.join(GOLDEN, f"urdf_{robot}.npz"), allow_pickle=False)
    v = lambda a: quoteattr(" ".join(repr(float(x)) for x in a))
    out = [f"<robot name={quoteattr(str(t['robot_name']))}>"]
    for i, name in enumerate(t["link_name"]):
        rpy = f" rpy={v(t['link_com_rpy'][i])}" if t["link_has_com_rpy"][i] else ""
        out.append(f"<link name={quoteattr(str(name))}><inertial><origin xyz={v(t['link_com'][i])}{rpy}/>"
                   f"<mass value={quoteattr(repr(float(t['link_mass'][i])))}/>")
        if t["link_has_inertia"][i]:
            out.append("<inertia " + " ".join(f"{k}={quoteattr(repr(float(x)))}" for k, x in zip(("ixx", "ixy", "ixz", "iyy", "iyz", "izz"), t["link_inertia"][i])) + "/>")
        out.append("</inertial></link>")
    for i, name in enumerate(t["joint_name"]):
        axis = f"<axis xyz={v(t['joint_axis'][i])}/>" if t["joint_has_axis"][i] else ""
        out.append(f"<joint name={quoteattr(str(name))} type={quoteattr(str(t['joint_type'][i]))}><origin xyz={v(t['joint_xyz'][i])} rpy={v(t['joint_rpy'][i])}/>"
                   f"<parent link={quoteattr(str(t['joint_parent'][i]))}/><child link={quoteattr(str(t['joint_child'][i]))}/>{axis}</joint>")
    out.append("</robot>")
    path = os.path.join(str(dest), robot + ".urdf")
    with open(path, "w") as f:
        f.write("\n".join(out))
    return path


@pytest.mark.parametrize("urdf", ["quadruped_robot_v2", "quadfinger"])
def test_loop_closure_against_urdf(urdf, tmp_path):
    """The analytic embedding closes the removed closed_chain_revolute joints of the URDF to < 0.05 mm
    over the whole admissible range of D = dof2 - dof3 (reset window 0.384..2.61)."""
    from locomanipulationrl_amd.model.urdf import parse_urdf, build_tree, forward_kinematics, loop_residual
    links, joints = parse_urdf(_urdf_from_golden(urdf, tmp_path))
    tree = build_tree(links, joints)
    assert len(tree.loops) == 4 and len(tree.bodies) == 21
    rng = np.random.default_rng(0)
    for D in np.linspace(0.3, 2.8, 12):
        q = {}
        for mod in ("a1", "a2", "a3", "a4"):
            q2 = rng.uniform(-1, 1); g, _, _ = closure_g(D)
            q[f"{mod}-dof1"] = rng.uniform(-1, 1); q[f"{mod}-dof2"] = q2; q[f"{mod}-dof3"] = q2 - D
            for b in tree.bodies:
                if b.joint_name.startswith(f"{mod}-link4_to_link3"):
                    q[b.joint_name] = g
                if b.joint_name.startswith(f"{mod}-link1_to_link2"):
                    q[b.joint_name] = -g
        poses = forward_kinematics(tree, q)
        for lp in tree.loops:
            gap, ang = loop_residual(tree, poses, lp)
            assert gap < 5e-5 and ang < 1e-4, (urdf, D, lp.name, gap, ang)


def test_compiled_assets_are_current(robot_model, tmp_path):
    from locomanipulationrl_amd.model.robot_model import compile_urdf
    m = compile_urdf(_urdf_from_golden("quadruped_robot_v2", tmp_path))
    for k in ("Rt", "pt", "mass", "com", "inertia", "tip_off"):
        assert np.allclose(getattr(m, k), getattr(robot_model, k), atol=1e-12)
    assert list(m.dof) == list(robot_model.dof)


def test_packed_table_layout(robot_model):
    t = robot_model.packed_table()
    assert t.dtype == np.float32 and t.shape == (HUB_FLOATS + 4 * LIMB_STRIDE,)
    assert abs(t[0] - robot_model.mass[0]) < 1e-6
    # every joint rotation block is orthonormal, every axis sign is +-1
    for l in range(4):
        o = HUB_FLOATS + l * LIMB_STRIDE
        for j in range(5):
            R = t[o + 13 * j: o + 13 * j + 9].reshape(3, 3).astype(np.float64)
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6
            assert abs(abs(t[o + 13 * j + 12]) - 1) < 1e-7


def test_foot_collider_is_the_mesh_hemisphere(robot_model, vertical_model):
    """The foot sphere of the model (robot_model.py FOOT_*) is the far end of the reference's own collision meshes: the hull vertices of
    Design/RobotURDF/mesh/collision/overconstrained/{link3,link2_right}.obj beyond y = -122.5 mm (tests/golden/foot_hull.npz) lie on a
    sphere of radius 5 mm about the model's contact offsets; the fingertip frame the task reads is that sphere's apex; on the horizontal
    robot the four spheres are mirror images of each other although the reference's fingertip frames are not."""
    from conftest import GOLDEN
    from locomanipulationrl_amd.model.robot_model import FOOT_CENTRE_LEFT, FOOT_CENTRE_RIGHT, FOOT_RADIUS
    g = np.load(os.path.join(GOLDEN, "foot_hull.npz"))
    for name, c in (("link3", FOOT_CENTRE_LEFT), ("link2_right", FOOT_CENTRE_RIGHT)):
        v = g[name]
        assert v.shape == (121, 3)
        r = np.linalg.norm(v - np.array(c), axis=1)
        assert np.abs(r - FOOT_RADIUS).max() < 2e-6, (name, np.abs(r - FOOT_RADIUS).max())          # 6-digit mesh coordinates
        assert abs(g[name + "_aabb"][0, 1] + 0.127) < 1e-9                                            # the link ends at the fingertip frame's y
    assert np.allclose(np.array(FOOT_CENTRE_LEFT) + [0, -FOOT_RADIUS, 0], robot_model.tip_off[0], atol=1e-9)      # apex = fingertip_frame
    # horizontal robot: left-hand modules carry the sphere on link3, right-hand ones on link2 (the long link of that module)
    names = robot_model.body_names
    for l in range(4):
        right = names[int(robot_model.limb_body_index[l, 2])].endswith("_right")
        assert int(robot_model.contact_body[l]) == int(robot_model.limb_body_index[l, 4 if right else 2])
    q = [-1.2, 1.2, 1.2, -1.2, -1.22, -1.92, 1.92, 1.22, 1.92, 1.22, -1.22, -1.92]
    c = robot_model.foot_centres(q)
    assert np.abs(c[0] * [-1, 1, 1] - c[1]).max() < 2e-5 and np.abs(c[2] * [-1, 1, 1] - c[3]).max() < 2e-5          # a1 <-> a2, a3 <-> a4 mirror in x
    t = robot_model.tip_positions(q)
    assert abs(t[0, 1] - 0.1223) < 1e-4 and abs(t[1, 1] - 0.1408) < 1e-4                                            # the frames are not (known answer)
    # vertical robot: four left-hand modules
    assert all(int(vertical_model.contact_body[l]) == int(vertical_model.limb_body_index[l, 2]) for l in range(4))
    # the packed table carries the sphere: centre at +118..120, body flag at +121 of each limb block
    tb = robot_model.packed_table()
    for l in range(4):
        o = HUB_FLOATS + l * LIMB_STRIDE
        assert np.allclose(tb[o + 118: o + 121], robot_model.contact_off[l], atol=1e-7) and tb[o + 121] == (1.0 if l in (1, 3) else 0.0)


def test_plate_intersection_census_geometry():
    """tools/plate_intersection.py (how often the plate passes through bodies that have no collider here): its batched forward
    kinematics equals RobotModel.fk, and its three flags answer the known cases of a flipped plate lowered onto the inverted robot - resting on
    the feet: nothing; through the links but above the frame: hull and axis; inside the frame box: all three."""
    import sys
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import plate_intersection as PI
    from locomanipulationrl_amd.engine_config import mani_params
    from locomanipulationrl_amd.model.robot_model import load_model
    rm = load_model("quadruped_robot_v2"); geo = PI.Geometry(rm, "cpu"); ep = mani_params()
    q = np.array(ep.init_q) + 0.1 * np.random.default_rng(0).standard_normal(12)
    Rb = PI.quat_to_mat(torch.tensor([ep.fixed_base_quat])); pb = torch.tensor([ep.fixed_base_pos])
    R, p = geo.body_poses(torch.tensor(q[None], dtype=torch.float32), Rb, pb)
    ref = rm.fk(q, Rb[0].numpy().astype(float), pb[0].numpy().astype(float))
    assert max(np.abs(p[k][0].numpy() - ref[k][1]).max() for k in range(rm.nb)) < 1e-6
    st = torch.zeros(115, 3); st[13:25] = torch.tensor(ep.init_q)[:, None]; st[40:44] = torch.tensor(ep.init_plate_quat)[:, None]
    st[39] = torch.tensor([0.14, 0.05, 0.02])                      # plate origin heights: on the feet / among the links / inside the frame
    frame, hull, axis, rim = (x.tolist() for x in geo.flags(st, ep, slice(0, 3)))
    assert frame == [False, False, True] and hull == [False, True, True] and axis == [False, True, True] and rim == [False, False, False]
