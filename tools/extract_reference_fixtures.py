#!/usr/bin/env python3
"""Numeric fixtures taken from the reference's own data files (build container only; /root/reference never ships).

  tests/golden/npy_traj.npz   the 13 PhysX joint-position recordings RobotLearning/omniisaacgymenvs/tasks/joint_train_locomanipulation/*.npy
                              (written by joint_locomanipulation.py:556-563,861-874: env 0 of the locomotion half / of the manipulation
                              robot view, one row per control step from the reset step until that env's reset flag is raised), float32 (T, 12)
  tests/golden/foot_hull.npz  the convex-hull vertices of the far end (y < -122.5 mm) of the two long distal links' collision meshes
                              Design/RobotURDF/mesh/collision/overconstrained/{link3,link2_right}.obj, metres, link frame
  tests/golden/urdf_{quadruped_robot_v2,quadfinger}.npz
                              the kinematic and inertial tables of Design/RobotURDF/robot_urdfs/<robot>.urdf, in document order: per link
                              its name, mass, inertial origin (xyz, rpy) and inertia (ixx ixy ixz iyy iyz izz); per joint its name, type,
                              parent, child, origin (xyz, rpy) and axis; `*_has_*` flags mark the elements / attributes the URDF omits
                              (tests/test_model.py writes a URDF with only these elements back from them and compiles it)

Arrays only (numpy.load(allow_pickle=False) / a four-token text parse of the OBJ `v` records); no reference source text is stored.
"""
import glob
import os
import xml.etree.ElementTree as ET

import numpy as np
from scipy.spatial import ConvexHull

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def obj_vertices(path):
    v = [[float(x) for x in line.split()[1:4]] for line in open(path, errors="ignore") if line.startswith("v ")]
    return np.asarray(v, dtype=np.float64) * 1e-3          # the xacro scales the meshes by 0.001 (overconstrained_parts.xacro:4)


def urdf_tables(path):
    """The numbers model/urdf.py:parse_urdf reads from a URDF, as arrays (visual / collision geometry is not read and not kept)."""
    root = ET.parse(path).getroot()
    vec = lambda e, k: [float(x) for x in e.get(k).split()] if e is not None and e.get(k) is not None else [0.0, 0.0, 0.0]
    links, joints = root.findall("link"), root.findall("joint")
    for le in links:        # every link of these robots carries <inertial> with <origin> and <mass>; only <inertia> / rpy may be absent
        assert le.find("inertial") is not None and le.find("inertial/origin") is not None and le.find("inertial/mass") is not None
    for je in joints:
        assert je.find("origin") is not None and je.find("origin").get("xyz") is not None and je.find("origin").get("rpy") is not None
    ine = [le.find("inertial/inertia") for le in links]
    return dict(
        robot_name=np.array(root.get("name")),
        link_name=np.array([le.get("name") for le in links]),
        link_mass=np.array([float(le.find("inertial/mass").get("value")) for le in links]),
        link_com=np.array([vec(le.find("inertial/origin"), "xyz") for le in links]),
        link_com_rpy=np.array([vec(le.find("inertial/origin"), "rpy") for le in links]),
        link_has_com_rpy=np.array([le.find("inertial/origin").get("rpy") is not None for le in links]),
        link_inertia=np.array([[float(e.get(k)) for k in ("ixx", "ixy", "ixz", "iyy", "iyz", "izz")] if e is not None else [0.0] * 6 for e in ine]),
        link_has_inertia=np.array([e is not None for e in ine]),
        joint_name=np.array([je.get("name") for je in joints]),
        joint_type=np.array([je.get("type") for je in joints]),
        joint_parent=np.array([je.find("parent").get("link") for je in joints]),
        joint_child=np.array([je.find("child").get("link") for je in joints]),
        joint_xyz=np.array([vec(je.find("origin"), "xyz") for je in joints]),
        joint_rpy=np.array([vec(je.find("origin"), "rpy") for je in joints]),
        joint_axis=np.array([vec(je.find("axis"), "xyz") for je in joints]),
        joint_has_axis=np.array([je.find("axis") is not None for je in joints]),
    )


def main():
    assert os.path.isdir(REF), "reference tree not present: fixtures can only be regenerated in the build container"
    d = os.path.join(REF, "RobotLearning/omniisaacgymenvs/tasks/joint_train_locomanipulation")
    traj = {os.path.basename(f)[:-4].replace("-", "_"): np.load(f, allow_pickle=False).astype(np.float32) for f in sorted(glob.glob(os.path.join(d, "*.npy")))}
    assert len(traj) == 13 and all(a.ndim == 2 and a.shape[1] == 12 for a in traj.values())
    np.savez_compressed(os.path.join(OUT, "npy_traj.npz"), **traj)
    print("npy_traj.npz:", {k: v.shape for k, v in traj.items()})
    hull = {}
    for name in ("link3", "link2_right"):
        v = obj_vertices(os.path.join(REF, "Design/RobotURDF/mesh/collision/overconstrained", name + ".obj"))
        hv = v[ConvexHull(v).vertices]
        hull[name] = hv[hv[:, 1] < -0.1225]
        hull[name + "_aabb"] = np.stack([v.min(0), v.max(0)])
    np.savez_compressed(os.path.join(OUT, "foot_hull.npz"), **hull)
    print("foot_hull.npz:", {k: v.shape for k, v in hull.items()})
    for robot in ("quadruped_robot_v2", "quadfinger"):
        t = urdf_tables(os.path.join(REF, "Design/RobotURDF/robot_urdfs", robot + ".urdf"))
        np.savez_compressed(os.path.join(OUT, f"urdf_{robot}.npz"), **t)
        print(f"urdf_{robot}.npz:", {k: v.shape for k, v in t.items()})


if __name__ == "__main__":
    main()
