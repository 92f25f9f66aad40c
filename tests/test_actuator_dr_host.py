"""Actuator randomisation, the host side: the YAML entries `articulation_views.<robot>.joint_kps`, `joint_kds` and
`command_latency` -> EngineParams.dr_actuator -> lm_actuator_dr, the refusals with their reasons, the C layout, and the guarantee that blocks
without the entries carry no actuator channel.  The refusals of lm_set_actuator_randomization that need a live handle are checked on the GPU
(tests/test_gpu_actuator_dr.py)."""
import ctypes as C
import dataclasses
import glob
import os
import subprocess
import tempfile
import warnings

import pytest

from conftest import ROOT
from locomanipulationrl_amd import lib as lmlib
from locomanipulationrl_amd.engine_config import (DR_ACTUATOR_CHANNELS, DR_ACTUATOR_KD, DR_ACTUATOR_KP, DR_ACTUATOR_LATENCY, DR_ACTUATOR_ROWS,
                                                  DR_DISTRIBUTIONS, DR_ON_STARTUP, DR_OPERATIONS, DR_STREAM_ACTUATOR, DRChannel, EngineParams, loco_params)
from locomanipulationrl_amd.utils.config import SimConfig, load_config
from locomanipulationrl_amd.utils.task_util import task_map

TASKS = sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(ROOT, "locomanipulationrl_amd", "cfg", "task", "*.yaml")))
LOCO, MANI, LOCO_CC, MANI_CC, LOCO_PC, BOTH, BOTH_PC = ("QuadrupedPoseControl", "QuadrupedManipulatePlate", "QuadrupedPoseControlCustomController",
                                                        "QuadrupedManipulatePlateCustomController", "QuadrupedPoseControlPositionControl",
                                                        "JointLocomanipulation", "JointLocomanipulationPositionControl")


def task_of(name, params=None, randomize=True, control_mode=None):
    cfg = load_config(name, num_envs=32)
    dr = cfg["task"].setdefault("domain_randomization", {})
    dr["randomize"] = randomize
    if params is not None:
        dr["randomization_params"] = params
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t = task_map()[name](name=name, sim_config=SimConfig(cfg), env=None)
    if control_mode is not None:          # RobotOmni's other two control modes (variant 0): position (kp 5, kd 1) / effort
        rd = t.robot_locomotion.robot_description
        rd.control_mode = control_mode; rd.joint_kps = [5, 5, 5] * 4; rd.joint_kds = [1, 1, 1] * 4
    return t


def blocks(name, params=None, randomize=True, control_mode=None):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return task_of(name, params, randomize, control_mode).engine_params()


def entry(trigger, prm, op="scaling", dist="uniform", interval=3):
    e = dict(operation=op, distribution=dist, distribution_parameters=prm)
    if trigger == "on_interval":
        e["frequency_interval"] = interval
    return {trigger: e}


def robot(**attrs):
    return {"articulation_views": {"robot_view": attrs}}


def is_channel(ch, op, dist, interval, lo, hi):
    return (ch.enabled == 1 and ch.operation == DR_OPERATIONS[op] and ch.distribution == DR_DISTRIBUTIONS[dist] and ch.interval == interval
            and ch.p0[0] == lo and ch.p1[0] == hi)


def all_off(ep):
    return len(ep.dr_actuator) == DR_ACTUATOR_CHANNELS and not any(ch.enabled for ch in ep.dr_actuator)


TRIGGERS = [("on_startup", DR_ON_STARTUP), ("on_reset", 0), ("on_interval", 3)]


@pytest.mark.parametrize("trigger,interval", TRIGGERS)
def test_joint_kps_parses_with_each_trigger(trigger, interval):
    t = task_of(LOCO_CC, robot(joint_kps=entry(trigger, [0.5, 2.0], dist="loguniform")))
    (ep,) = t.engine_params()
    assert ep.variant == 1 and ep.dr_enabled == 1 and (ep.pd_kp, ep.kd) == (4.5, 0.2)
    assert is_channel(ep.dr_actuator[DR_ACTUATOR_KP], "scaling", "loguniform", interval, 0.5, 2.0)
    assert not ep.dr_actuator[DR_ACTUATOR_KD].enabled and not ep.dr_actuator[DR_ACTUATOR_LATENCY].enabled
    assert ("articulation_views", "robot_view", "joint_kps", trigger) in t._dr_randomizer.active_domain_randomizations
    (ep,) = blocks(LOCO_PC, robot(joint_kps=entry(trigger, [0.0, 1.0], "additive", "gaussian")))          # a gaussian tail is floored, not refused
    assert ep.variant == 2 and is_channel(ep.dr_actuator[DR_ACTUATOR_KP], "additive", "gaussian", interval, 0.0, 1.0)
    (ep,) = blocks(LOCO, robot(joint_kps=entry(trigger, [2.0, 8.0], "direct")), control_mode="position")          # variant 0 in position drive mode
    assert ep.variant == 0 and ep.drive_mode == 1 and is_channel(ep.dr_actuator[DR_ACTUATOR_KP], "direct", "uniform", interval, 2.0, 8.0)


@pytest.mark.parametrize("trigger,interval", TRIGGERS)
def test_joint_kds_parses_with_each_trigger(trigger, interval):
    for name in (LOCO, MANI, LOCO_CC, MANI_CC, LOCO_PC):          # every family: the velocity drive too
        (ep,) = blocks(name, robot(joint_kds=entry(trigger, [0.5, 2.0])))
        assert is_channel(ep.dr_actuator[DR_ACTUATOR_KD], "scaling", "uniform", interval, 0.5, 2.0), name
        assert not ep.dr_actuator[DR_ACTUATOR_KP].enabled and not ep.dr_actuator[DR_ACTUATOR_LATENCY].enabled
    (ep,) = blocks(LOCO, robot(joint_kds=entry(trigger, [50.0, 200.0], "direct", "loguniform")))
    assert ep.kd == 100.0 and is_channel(ep.dr_actuator[DR_ACTUATOR_KD], "direct", "loguniform", interval, 50.0, 200.0)
    (ep,) = blocks(LOCO, robot(joint_kds=entry(trigger, [0.5, 2.0])), control_mode="position")
    assert ep.drive_mode == 1 and ep.dr_actuator[DR_ACTUATOR_KD].enabled


@pytest.mark.parametrize("trigger,interval", TRIGGERS)
def test_command_latency_parses_with_each_trigger(trigger, interval):
    for name in (LOCO_CC, MANI_CC, LOCO_PC):
        t = task_of(name, robot(command_latency=entry(trigger, [0.0, 6.0], "additive")))
        (ep,) = t.engine_params()
        assert ep.variant >= 1 and is_channel(ep.dr_actuator[DR_ACTUATOR_LATENCY], "additive", "uniform", interval, 0.0, 6.0), name
        assert ("articulation_views", "robot_view", "command_latency", trigger) in t._dr_randomizer.active_domain_randomizations
    (ep,) = blocks(LOCO_CC, robot(command_latency=entry(trigger, [1.0, 0.5], "direct", "gaussian")))
    assert is_channel(ep.dr_actuator[DR_ACTUATOR_LATENCY], "direct", "gaussian", interval, 1.0, 0.5)


def test_the_three_entries_together_reach_the_c_struct():
    prm = robot(joint_kps=entry("on_startup", [0.5, 2.0], dist="loguniform"), joint_kds=entry("on_reset", [-0.05, 0.1], "additive"),
                command_latency=entry("on_interval", [0.0, 6.0], "direct", interval=7))
    (ep,) = blocks(LOCO_CC, prm)
    ad = lmlib.make_actuator_dr(ep)
    assert (ad.ch[DR_ACTUATOR_KP].enabled, ad.ch[DR_ACTUATOR_KP].interval, ad.ch[DR_ACTUATOR_KP].distribution) == (1, DR_ON_STARTUP, DR_DISTRIBUTIONS["loguniform"])
    assert (ad.ch[DR_ACTUATOR_KD].enabled, ad.ch[DR_ACTUATOR_KD].interval, ad.ch[DR_ACTUATOR_KD].operation) == (1, 0, DR_OPERATIONS["additive"])
    assert (ad.ch[DR_ACTUATOR_LATENCY].enabled, ad.ch[DR_ACTUATOR_LATENCY].interval, ad.ch[DR_ACTUATOR_LATENCY].operation) == (1, 7, DR_OPERATIONS["direct"])
    assert abs(ad.ch[DR_ACTUATOR_KD].p0[0] + 0.05) < 1e-7 and abs(ad.ch[DR_ACTUATOR_LATENCY].p1[0] - 6.0) < 1e-7
    assert lmlib.make_params(ep).dr_enabled == 1          # the parameter block itself does not carry them
    from oracle import lmo
    assert lmo.make_params(ep).dr_enabled == 1            # the oracle's make_params works on a block that carries the field


def test_cotraining_blocks_both_carry_the_channels():
    prm = robot(joint_kds=entry("on_startup", [0.5, 2.0]))
    lo, ma = blocks(BOTH, prm)
    for ep in (lo, ma):
        assert ep.variant == 0 and is_channel(ep.dr_actuator[DR_ACTUATOR_KD], "scaling", "uniform", DR_ON_STARTUP, 0.5, 2.0)
    prm = robot(joint_kps=entry("on_reset", [0.5, 2.0]), command_latency=entry("on_interval", [0.0, 6.0], "additive"))
    lo, ma = blocks(BOTH_PC, prm)
    for ep in (lo, ma):
        assert ep.variant == 2 and ep.dr_actuator[DR_ACTUATOR_KP].enabled and ep.dr_actuator[DR_ACTUATOR_LATENCY].enabled


NAN = float("nan")
REFUSALS = [
    # (task, control mode, randomization_params, exception, text the message must carry)
    (LOCO_CC, None, robot(joint_kps={**entry("on_reset", [0.5, 2.0]), **entry("on_interval", [0.5, 2.0])}), NotImplementedError, "joint_kps"),          # two triggers
    (LOCO_CC, None, robot(joint_kds={**entry("on_startup", [0.5, 2.0]), **entry("on_reset", [0.5, 2.0])}), NotImplementedError, "joint_kds"),
    (LOCO_CC, None, robot(command_latency={**entry("on_startup", [0, 3], "additive"), **entry("on_interval", [0, 3], "additive")}), NotImplementedError, "command_latency"),
    (LOCO_CC, None, robot(joint_kps={}), NotImplementedError, "exactly one"),                                   # no trigger
    (LOCO, None, robot(joint_kps=entry("on_reset", [0.5, 2.0])), NotImplementedError, "no position gain"),      # velocity drive
    (MANI, None, robot(joint_kps=entry("on_startup", [0.5, 2.0])), NotImplementedError, "no position gain"),
    (BOTH, None, robot(joint_kps=entry("on_startup", [0.5, 2.0])), NotImplementedError, "no position gain"),
    (LOCO, "effort", robot(joint_kps=entry("on_reset", [0.5, 2.0])), NotImplementedError, "no position gain"),
    (LOCO, "effort", robot(joint_kds=entry("on_reset", [0.5, 2.0])), NotImplementedError, "gains off"),
    (LOCO, None, robot(command_latency=entry("on_reset", [0.0, 4.0], "additive")), NotImplementedError, "PD-actuator tasks only"),      # variant 0
    (MANI, None, robot(command_latency=entry("on_startup", [0.0, 4.0], "direct")), NotImplementedError, "PD-actuator tasks only"),
    (LOCO, "position", robot(command_latency=entry("on_reset", [0.0, 4.0], "additive")), NotImplementedError, "PD-actuator tasks only"),
    (LOCO_CC, None, robot(command_latency=entry("on_reset", [0.0, 4.0], "scaling")), ValueError, "nominal latency is 0"),
    (LOCO_CC, None, robot(joint_kps=entry("on_reset", [0.0, 2.0])), ValueError, "non-positive"),                 # scaling by U(0, 2) reaches 0
    (LOCO_CC, None, robot(joint_kps=entry("on_reset", [-4.5, 1.0], "additive")), ValueError, "non-positive"),    # 4.5 - 4.5
    (LOCO_CC, None, robot(joint_kds=entry("on_reset", [-0.2, 0.2], "additive")), ValueError, "non-positive"),    # 0.2 - 0.2
    (LOCO_PC, None, robot(joint_kds=entry("on_startup", [-0.1, 0.3], "direct")), ValueError, "non-positive"),
    (LOCO, None, robot(joint_kds=entry("on_interval", [-1.0, 2.0])), ValueError, "non-positive"),
    (LOCO_CC, None, robot(joint_kps=entry("on_reset", [0.5, NAN])), ValueError, "finite"),
    (LOCO_CC, None, robot(joint_kds=entry("on_reset", [float("inf"), 1.0], "additive", "gaussian")), ValueError, "finite"),
    (LOCO_CC, None, robot(command_latency=entry("on_reset", [0.0, NAN], "additive")), ValueError, "finite"),
    (LOCO_CC, None, robot(joint_kps=entry("on_reset", [0.0, 2.0], dist="loguniform")), ValueError, "loguniform"),
    (LOCO_CC, None, robot(joint_kds=entry("on_reset", [-1.0, 2.0], dist="loguniform")), ValueError, "loguniform"),
    (LOCO_CC, None, robot(command_latency=entry("on_reset", [0.0, 4.0], "additive", "loguniform")), ValueError, "loguniform"),
    (LOCO_CC, None, robot(joint_kps=entry("on_reset", [[0.5] * 12, [2.0] * 12])), ValueError, "one draw per env"),          # per-joint gains: out of scope
    (LOCO_CC, None, robot(joint_kds=entry("on_reset", [0.5, 1.0, 2.0])), ValueError, "[a, b]"),
    (LOCO_CC, None, robot(joint_kps=entry("on_interval", [0.5, 2.0], interval=0)), ValueError, "frequency_interval"),
    (LOCO_CC, None, robot(joint_kds={"on_interval": dict(operation="scaling", distribution="uniform", distribution_parameters=[0.5, 2.0])}), ValueError, "frequency_interval"),
    (LOCO_CC, None, robot(joint_kps=entry("on_reset", [0.5, 2.0], op="multiply")), ValueError, "joint_kps"),
    (LOCO_CC, None, robot(command_latency=entry("on_reset", [0.0, 4.0], "additive", "poisson")), ValueError, "command_latency"),
    (LOCO_CC, None, robot(joint_kds=None), ValueError, "joint_kds"),
    (LOCO_CC, None, robot(stiffness=entry("on_reset", [0.5, 2.0])), NotImplementedError, "stiffness"),          # the OIGE entry stays refused
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_refusals_name_the_reason(case):
    name, mode, prm, exc, text = REFUSALS[case]
    with pytest.raises(exc) as ei:
        blocks(name, prm, control_mode=mode)
    assert text in str(ei.value), str(ei.value)


def test_a_positive_bounded_range_and_a_gaussian_are_accepted():
    (ep,) = blocks(LOCO_CC, robot(joint_kds=entry("on_reset", [-0.19, 0.2], "additive")))          # 0.2 - 0.19 stays positive
    assert ep.dr_actuator[DR_ACTUATOR_KD].enabled
    (ep,) = blocks(LOCO_CC, robot(joint_kds=entry("on_reset", [0.0, 5.0], "additive", "gaussian")))          # a wide gaussian: the floor's business
    assert ep.dr_actuator[DR_ACTUATOR_KD].enabled
    (ep,) = blocks(LOCO_CC, robot(command_latency=entry("on_reset", [-3.0, 20.0], "additive")))          # the latency is clamped to [0, sub-steps], not refused
    assert ep.dr_actuator[DR_ACTUATOR_LATENCY].enabled


def test_gain_range_is_checked_against_the_blocks_own_gains():
    """additive U(-0.15, 0.1) keeps the shipped kd = 0.2 positive and is accepted; the same entry on a block built with kd = 0.1 is refused."""
    t = task_of(LOCO_CC, robot(joint_kds=entry("on_reset", [-0.15, 0.1], "additive")))
    (ep,) = t.engine_params()
    assert ep.kd == 0.2 and ep.dr_actuator[DR_ACTUATOR_KD].enabled
    with pytest.raises(ValueError, match="non-positive"):
        t._common(t.robot_locomotion, kd=0.1)
    assert t._common(t.robot_locomotion, kd=0.5).dr_actuator[DR_ACTUATOR_KD].enabled


def test_actuator_struct_matches_the_header():
    """lm_actuator_dr is three lm_dr_channel; lm_params, the ABI number and LM_DR_PHYS_ROWS are what they were."""
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "lm_engine.h"\nint main(){printf("%zu %zu %d %d %d %d %d %zu %d %d %d %d %d\\n", sizeof(lm_actuator_dr), '
           'offsetof(lm_actuator_dr, ch[2]), LM_DR_ACTUATOR_CHANNELS, LM_DR_ACTUATOR_ROWS, (int)LM_PTR_DR_ACTUATOR, LM_ABI_VERSION, LM_DR_PHYS_ROWS, '
           'sizeof(lm_params), LM_DR_ACTUATOR_KP, LM_DR_ACTUATOR_KD, LM_DR_ACTUATOR_LATENCY, (int)LM_PTR_CONTACT, (int)LM_PTR_DR_MASS);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c"); open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = list(map(int, subprocess.check_output([exe]).split()))
    size, off2, nch, rows, kind, abi, phys_rows, psize = out[:8]
    A = lmlib.LmActuatorDr
    assert (size, off2) == (C.sizeof(A), 2 * C.sizeof(lmlib.LmDrChannel)) == (3 * C.sizeof(lmlib.LmDrChannel), 2 * C.sizeof(lmlib.LmDrChannel))
    assert (nch, rows, kind) == (lmlib.DR_ACTUATOR_CHANNELS, lmlib.DR_ACTUATOR_ROWS, lmlib.PTR_DR_ACTUATOR) == (3, 3, 13)
    assert (DR_ACTUATOR_CHANNELS, DR_ACTUATOR_ROWS, DR_STREAM_ACTUATOR) == (3, 3, 19)
    assert (abi, phys_rows, psize) == (5, 43, C.sizeof(lmlib.LmParams)) and lmlib.ABI_VERSION == 5 and lmlib.DR_PHYS_ROWS == 43
    assert C.sizeof(lmlib.LmParams) == 1404          # sizeof(lm_params) before the actuator channels existed
    assert tuple(out[8:11]) == (DR_ACTUATOR_KP, DR_ACTUATOR_KD, DR_ACTUATOR_LATENCY) == (0, 1, 2)
    assert tuple(out[11:]) == (lmlib.PTR_CONTACT, lmlib.PTR_DR_MASS) == (12, 11)          # the earlier kinds keep their numbers


def test_without_the_entries_no_actuator_channel_is_on():
    """Every shipped task, randomisation on and off: dr_actuator is all off, and so is the C struct made from it."""
    for name in TASKS:
        for dr in (False, True):
            for ep in blocks(name, None, randomize=dr):
                assert all_off(ep), (name, dr)
                assert not any(c.enabled for c in lmlib.make_actuator_dr(ep).ch)
    assert all_off(EngineParams()) and all_off(loco_params(dr_enabled=1))
    assert not any(c.enabled for c in lmlib.make_actuator_dr(loco_params()).ch)


def test_blocks_without_the_entries_are_what_they_were():
    """A block built from a YAML without actuator entries carries the all-off default in its one new field, and the C parameter block does not
    depend on that field: byte for byte the same with a channel switched on in it (the channels travel in lm_actuator_dr alone)."""
    on = DRChannel(enabled=1, operation=DR_OPERATIONS["scaling"], distribution=DR_DISTRIBUTIONS["uniform"], interval=0, p0=[0.5] * 3, p1=[2.0] * 3)
    for name in (LOCO, LOCO_CC, BOTH_PC):
        for ep in blocks(name, None, randomize=True):
            assert ep.dr_actuator == EngineParams().dr_actuator == [DRChannel()] * DR_ACTUATOR_CHANNELS
            twin = dataclasses.replace(ep, dr_actuator=[on, on, DRChannel()])
            assert bytes(lmlib.make_params(ep)) == bytes(lmlib.make_params(twin))
    assert "dr_actuator" not in {f[0] for f in lmlib.LmParams._fields_}
    assert [f.name for f in dataclasses.fields(EngineParams)].count("dr_actuator") == 1


def test_entry_point_refuses_null_arguments_without_a_gpu():
    """lm_set_actuator_randomization needs a live handle for everything else (an engine exists only on a GPU): those refusals are in
    tests/test_gpu_actuator_dr.py::test_entry_point_refusals."""
    so = lmlib.load_library() if os.path.exists(lmlib._SO) else (lmlib.build_library(), lmlib.load_library())[1]
    assert "lm_set_actuator_randomization" in lmlib.EXPORTS
    ad = lmlib.LmActuatorDr()
    assert so.lm_set_actuator_randomization(None, 0, C.byref(ad)) == -1 and b"lm_set_actuator_randomization" in so.lm_last_error()
