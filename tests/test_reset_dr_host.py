"""Reset-state randomisation, the host side: the four YAML entries `joint_positions`, `joint_velocities`, `position`, `orientation`
-> EngineParams.dr_reset -> lm_reset_dr, the refusals, and the guarantee that blocks without the entries are what they were.  The refusals of
lm_set_reset_randomization that need a live handle are checked on the GPU (tests/test_gpu_reset_dr.py): only the null-argument ones are reachable here."""
import ctypes as C
import dataclasses
import glob
import json
import os
import subprocess
import tempfile
import warnings

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from locomanipulationrl_amd import lib as lmlib
from locomanipulationrl_amd.engine_config import (DR_DISTRIBUTIONS, DR_OPERATIONS, DR_RESET_CHANNELS, DR_RESET_JOINT_POS, DR_RESET_JOINT_VEL,
                                                  DR_RESET_ORIENTATION, DR_RESET_POSITION, DRChannel, EngineParams, MODE_LOCO, MODE_MANI, loco_params)
from locomanipulationrl_amd.utils.config import SimConfig, load_config
from locomanipulationrl_amd.utils.task_util import task_map

TASKS = sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(ROOT, "locomanipulationrl_amd", "cfg", "task", "*.yaml")))
LOCO, MANI, BOTH = "QuadrupedPoseControl", "QuadrupedManipulatePlate", "JointLocomanipulation"


def blocks(name, params=None, randomize=True):
    """EngineParams blocks of a shipped task with `params` as its whole randomization_params block."""
    cfg = load_config(name, num_envs=32)
    dr = cfg["task"].setdefault("domain_randomization", {})
    dr["randomize"] = randomize
    if params is not None:
        dr["randomization_params"] = params
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return task_map()[name](name=name, sim_config=SimConfig(cfg), env=None).engine_params()


def on_reset(prm, op="additive", dist="uniform"):
    return {"on_reset": dict(operation=op, distribution=dist, distribution_parameters=prm)}


# the reference's draws (quadruped_pose_control_custom_controller_dr.py, reset_idx)
JP, JV = on_reset([-0.1, 0.1]), on_reset([-0.1, 0.1])
POS = on_reset([[-0.05, -0.05, 0.0], [0.05, 0.05, 0.1]])
ORI = on_reset([[-0.1, -0.1, -1.2], [0.1, 0.1, 1.2]])


def robot(**attrs):
    return {"articulation_views": {"robot_view": attrs}}


def plate(**attrs):
    return {"rigid_prim_views": {"plate": attrs}}


def is_channel(ch, op, dist, p0, p1):
    return (ch.enabled == 1 and ch.operation == DR_OPERATIONS[op] and ch.distribution == DR_DISTRIBUTIONS[dist] and ch.interval == 0
            and list(ch.p0) == list(p0) and list(ch.p1) == list(p1))


def all_off(ep):
    return len(ep.dr_reset) == DR_RESET_CHANNELS and not any(ch.enabled for ch in ep.dr_reset)


def test_entries_parse_on_a_locomotion_task():
    (ep,) = blocks(LOCO, robot(joint_positions=JP, joint_velocities=JV, position=POS, orientation=ORI))
    assert ep.mode == MODE_LOCO and ep.dr_enabled == 1
    assert is_channel(ep.dr_reset[DR_RESET_JOINT_POS], "additive", "uniform", [-0.1] * 3, [0.1] * 3)
    assert is_channel(ep.dr_reset[DR_RESET_JOINT_VEL], "additive", "uniform", [-0.1] * 3, [0.1] * 3)
    assert is_channel(ep.dr_reset[DR_RESET_POSITION], "additive", "uniform", [-0.05, -0.05, 0.0], [0.05, 0.05, 0.1])
    assert is_channel(ep.dr_reset[DR_RESET_ORIENTATION], "additive", "uniform", [-0.1, -0.1, -1.2], [0.1, 0.1, 1.2])
    # one entry alone leaves the other three off; the other operations and distributions go through
    (ep,) = blocks(LOCO, robot(joint_positions=on_reset([0.9, 1.1], "scaling", "loguniform")))
    assert is_channel(ep.dr_reset[DR_RESET_JOINT_POS], "scaling", "loguniform", [0.9] * 3, [1.1] * 3)
    assert sum(ch.enabled for ch in ep.dr_reset) == 1
    (ep,) = blocks(LOCO, robot(orientation=on_reset([[0.0, 0.0, 0.5], [0.01, 0.01, 0.2]], "direct", "gaussian")))
    assert is_channel(ep.dr_reset[DR_RESET_ORIENTATION], "direct", "gaussian", [0.0, 0.0, 0.5], [0.01, 0.01, 0.2])


def test_entries_parse_on_a_manipulation_task():
    """The free body of a manipulation block is the plate: position / orientation are accepted under rigid_prim_views.plate."""
    prm = {**robot(joint_positions=JP, joint_velocities=JV), **plate(position=POS, orientation=ORI)}
    (ep,) = blocks(MANI, prm)
    assert ep.mode == MODE_MANI
    assert is_channel(ep.dr_reset[DR_RESET_JOINT_POS], "additive", "uniform", [-0.1] * 3, [0.1] * 3)
    assert is_channel(ep.dr_reset[DR_RESET_JOINT_VEL], "additive", "uniform", [-0.1] * 3, [0.1] * 3)
    assert is_channel(ep.dr_reset[DR_RESET_POSITION], "additive", "uniform", [-0.05, -0.05, 0.0], [0.05, 0.05, 0.1])
    assert is_channel(ep.dr_reset[DR_RESET_ORIENTATION], "additive", "uniform", [-0.1, -0.1, -1.2], [0.1, 0.1, 1.2])


def test_entries_parse_on_the_cotraining_task():
    """Two blocks: the joint entries reach both, the base's pose the locomotion block, the plate's pose the manipulation block."""
    ppos = on_reset([[0.0, 0.0, 0.0], [0.0, 0.0, 0.02]])
    prm = {"articulation_views": {"robot_view": dict(joint_positions=JP, joint_velocities=JV, position=POS, orientation=ORI)},
           "rigid_prim_views": {"plate": dict(position=ppos)}}
    lo, ma = blocks(BOTH, prm)
    assert (lo.mode, ma.mode) == (MODE_LOCO, MODE_MANI)
    for ep in (lo, ma):
        assert is_channel(ep.dr_reset[DR_RESET_JOINT_POS], "additive", "uniform", [-0.1] * 3, [0.1] * 3)
        assert is_channel(ep.dr_reset[DR_RESET_JOINT_VEL], "additive", "uniform", [-0.1] * 3, [0.1] * 3)
    assert is_channel(lo.dr_reset[DR_RESET_POSITION], "additive", "uniform", [-0.05, -0.05, 0.0], [0.05, 0.05, 0.1])
    assert is_channel(lo.dr_reset[DR_RESET_ORIENTATION], "additive", "uniform", [-0.1, -0.1, -1.2], [0.1, 0.1, 1.2])
    assert is_channel(ma.dr_reset[DR_RESET_POSITION], "additive", "uniform", [0.0, 0.0, 0.0], [0.0, 0.0, 0.02])
    assert not ma.dr_reset[DR_RESET_ORIENTATION].enabled


REFUSALS = [
    # (task, randomization_params, exception, text the message must carry)
    *[(LOCO, robot(**{a: {"on_interval": dict(frequency_interval=2, **e["on_reset"])}}), NotImplementedError, f"robot_view.{a}")
      for a, e in (("joint_positions", JP), ("joint_velocities", JV), ("position", POS), ("orientation", ORI))],
    *[(LOCO, robot(**{a: {"on_startup": dict(e["on_reset"])}}), NotImplementedError, f"robot_view.{a}")
      for a, e in (("joint_positions", JP), ("joint_velocities", JV), ("position", POS), ("orientation", ORI))],
    (MANI, plate(position={"on_interval": dict(frequency_interval=2, **POS["on_reset"])}), NotImplementedError, "plate.position"),
    (LOCO, robot(joint_velocities=on_reset([0.9, 1.1], "scaling")), ValueError, "robot_view.joint_velocities"),
    (LOCO, robot(orientation=on_reset([[0.9] * 3, [1.1] * 3], "scaling")), ValueError, "robot_view.orientation"),
    (MANI, plate(orientation=on_reset([[0.9] * 3, [1.1] * 3], "scaling")), ValueError, "plate.orientation"),
    (MANI, robot(position=POS), NotImplementedError, "robot_view.position"),          # the robot is fixed there
    (MANI, robot(orientation=ORI), NotImplementedError, "robot_view.orientation"),
    (LOCO, plate(position=POS), NotImplementedError, "plate.position"),               # no plate in a locomotion task
    (LOCO, plate(orientation=ORI), NotImplementedError, "plate.orientation"),
    (LOCO, robot(joint_positions=on_reset([0.0, 1.1], "scaling", "loguniform")), ValueError, "robot_view.joint_positions"),
    (LOCO, robot(position=on_reset([[1.0, 1.0, -1.0], [2.0, 2.0, 2.0]], "scaling", "loguniform")), ValueError, "robot_view.position"),
    (LOCO, robot(position=on_reset([-0.05, 0.05])), ValueError, "robot_view.position"),                    # needs per-component parameters
    (LOCO, robot(joint_positions=on_reset([[-0.1] * 3, [0.1] * 3])), ValueError, "robot_view.joint_positions"),      # scalar parameters
    (LOCO, robot(joint_positions=on_reset([-0.1, 0.1], "multiplicative")), ValueError, "robot_view.joint_positions"),
    (LOCO, robot(joint_positions={"on_reset": dict(operation="additive", distribution="uniform")}), ValueError, "robot_view.joint_positions"),
    (LOCO, robot(joint_positions=None), ValueError, "robot_view.joint_positions"),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_refusals_name_the_entry(case):
    name, prm, exc, text = REFUSALS[case]
    with pytest.raises(exc) as ei:
        blocks(name, prm)
    assert text in str(ei.value), str(ei.value)


def test_without_the_entries_the_blocks_are_unchanged():
    """Every shipped task, randomisation on and off: the EngineParams fields recorded from the earlier parameter block
    (tests/golden/engine_params_abi4.json) hold the same values, and all four reset-state channels are off."""
    ref = json.load(open(os.path.join(GOLDEN, "engine_params_abi4.json")))
    seen = 0
    for name in TASKS:
        for dr in (False, True):
            key = name + ("+dr" if dr else "")
            if key not in ref:
                continue
            eps = blocks(name, None, randomize=dr)
            assert len(eps) == len(ref[key])
            for ep, old in zip(eps, ref[key]):
                now = {k: v for k, v in dataclasses.asdict(ep).items() if k in old}
                assert set(old) <= set(now) and json.loads(json.dumps(now)) == old, key
                assert all_off(ep), key
            seen += 1
    assert seen == len(ref) and seen >= len(TASKS)
    assert all_off(EngineParams()) and all_off(loco_params(dr_enabled=1))


def test_min_frequency_zero_is_accepted_by_the_host():
    cfg = load_config(LOCO, num_envs=32)
    cfg["task"]["domain_randomization"].update(randomize=True, min_frequency=0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        (ep,) = task_map()[LOCO](name=LOCO, sim_config=SimConfig(cfg), env=None).engine_params()
    assert ep.dr_enabled == 1 and ep.dr_min_frequency == 0
    assert lmlib.make_params(ep).dr_min_frequency == 0


def test_reset_struct_matches_the_header():
    """lm_reset_dr is four lm_dr_channel; lm_params, the ABI number and LM_DR_PHYS_ROWS are what they were."""
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "lm_engine.h"\nint main(){printf("%zu %zu %d %d %d %d %d %zu\\n", sizeof(lm_reset_dr), '
           'offsetof(lm_reset_dr, ch[3]), LM_DR_RESET_CHANNELS, LM_DR_RESET_ROWS, (int)LM_PTR_DR_RESET_STATE, LM_ABI_VERSION, LM_DR_PHYS_ROWS, sizeof(lm_params));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c"); open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        size, off3, nch, rows, kind, abi, phys_rows, psize = map(int, subprocess.check_output([exe]).split())
    assert (size, off3) == (C.sizeof(lmlib.LmResetDr), 3 * C.sizeof(lmlib.LmDrChannel))
    assert (nch, rows, kind) == (lmlib.DR_RESET_CHANNELS, lmlib.DR_RESET_ROWS, lmlib.PTR_DR_RESET_STATE) == (4, 31, 10)
    assert (abi, phys_rows, psize) == (5, 43, C.sizeof(lmlib.LmParams))
    assert [(DR_RESET_JOINT_POS, DR_RESET_JOINT_VEL, DR_RESET_POSITION, DR_RESET_ORIENTATION)] == [(0, 1, 2, 3)]


def test_make_reset_dr_mirrors_the_channels_and_the_oracle_ignores_them():
    (ep,) = blocks(LOCO, robot(joint_positions=JP, orientation=ORI))
    rd = lmlib.make_reset_dr(ep)
    assert rd.ch[0].enabled == 1 and rd.ch[1].enabled == 0 and rd.ch[2].enabled == 0 and rd.ch[3].enabled == 1
    assert abs(rd.ch[0].p0[0] + 0.1) < 1e-7 and abs(rd.ch[3].p1[2] - 1.2) < 1e-7 and rd.ch[3].interval == 0
    assert lmlib.make_params(ep).dr_enabled == 1                      # the parameter block itself does not carry them
    assert not any(c.enabled for c in lmlib.make_reset_dr(loco_params()).ch)
    from oracle import lmo
    assert lmo.make_params(ep).dr_enabled == 1                        # the oracle's make_params works on a block that carries the field


def test_entry_point_refuses_null_arguments_without_a_gpu():
    """lm_set_reset_randomization needs a live handle for everything else (an engine exists only on a GPU): those refusals are in
    tests/test_gpu_reset_dr.py::test_entry_point_refusals."""
    so = lmlib.load_library() if os.path.exists(lmlib._SO) else (lmlib.build_library(), lmlib.load_library())[1]
    assert "lm_set_reset_randomization" in lmlib.EXPORTS
    rd = lmlib.LmResetDr()
    assert so.lm_set_reset_randomization(None, 0, C.byref(rd)) == -1 and b"lm_set_reset_randomization" in so.lm_last_error()
