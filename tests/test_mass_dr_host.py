"""Mass randomisation, the host side: the YAML entries `rigid_prim_views.plate.mass`, `rigid_prim_views.plate.density` and
`articulation_views.<robot>.body_masses` -> EngineParams.dr_mass (+ the per-body parameters in table order) -> lm_mass_dr, the refusals, the C
layout, and the guarantee that blocks without the entries carry no mass channel.  The refusals of lm_set_mass_randomization that need a live
handle are checked on the GPU (tests/test_gpu_mass_dr.py)."""
import ctypes as C
import glob
import os
import subprocess
import tempfile
import warnings

import numpy as np
import pytest

from conftest import ROOT
from locomanipulationrl_amd import lib as lmlib
from locomanipulationrl_amd.engine_config import (DR_DISTRIBUTIONS, DR_MASS_BODIES, DR_MASS_CHANNELS, DR_MASS_FLOOR, DR_MASS_PLATE, DR_MASS_PLATE_DENSITY,
                                                  DR_MASS_ROWS, DR_ON_STARTUP, DR_OPERATIONS, EngineParams, MODE_LOCO, MODE_MANI, loco_params)
from locomanipulationrl_amd.utils.config import SimConfig, load_config
from locomanipulationrl_amd.utils.task_util import task_map

TASKS = sorted(os.path.basename(p)[:-5] for p in glob.glob(os.path.join(ROOT, "locomanipulationrl_amd", "cfg", "task", "*.yaml")))
LOCO, MANI, BOTH, VERT = "QuadrupedPoseControl", "QuadrupedManipulatePlate", "JointLocomanipulation", "QuadrupedPoseControlVertical"


def task_of(name, params=None, randomize=True):
    cfg = load_config(name, num_envs=32)
    dr = cfg["task"].setdefault("domain_randomization", {})
    dr["randomize"] = randomize
    if params is not None:
        dr["randomization_params"] = params
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return task_map()[name](name=name, sim_config=SimConfig(cfg), env=None)


def blocks(name, params=None, randomize=True):
    """EngineParams blocks of a shipped task with `params` as its whole randomization_params block."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return task_of(name, params, randomize).engine_params()


def entry(trigger, prm, op="scaling", dist="uniform", interval=3):
    e = dict(operation=op, distribution=dist, distribution_parameters=prm)
    if trigger == "on_interval":
        e["frequency_interval"] = interval
    return {trigger: e}


def robot(e):
    return {"articulation_views": {"robot_view": {"body_masses": e}}}


def plate(**attrs):
    return {"rigid_prim_views": {"plate": attrs}}


def is_channel(ch, op, dist, interval, lo, hi):
    return (ch.enabled == 1 and ch.operation == DR_OPERATIONS[op] and ch.distribution == DR_DISTRIBUTIONS[dist] and ch.interval == interval
            and ch.p0[0] == lo and ch.p1[0] == hi)


def all_off(ep):
    return len(ep.dr_mass) == DR_MASS_CHANNELS and not any(ch.enabled for ch in ep.dr_mass)


@pytest.mark.parametrize("trigger,interval", [("on_startup", DR_ON_STARTUP), ("on_reset", 0), ("on_interval", 3)])
def test_plate_mass_parses_with_each_trigger(trigger, interval):
    (ep,) = blocks(MANI, plate(mass=entry(trigger, [0.5, 2.0])))
    assert ep.mode == MODE_MANI and ep.dr_enabled == 1
    assert is_channel(ep.dr_mass[DR_MASS_PLATE], "scaling", "uniform", interval, 0.5, 2.0)
    assert not ep.dr_mass[DR_MASS_PLATE_DENSITY].enabled and not ep.dr_mass[DR_MASS_BODIES].enabled
    (ep,) = blocks(MANI, plate(mass=entry(trigger, [0.0, 0.3], "additive", "gaussian")))          # a gaussian tail is floored, not refused
    assert is_channel(ep.dr_mass[DR_MASS_PLATE], "additive", "gaussian", interval, 0.0, 0.3)
    (ep,) = blocks(MANI, plate(mass=entry(trigger, [1.0, 4.0], "direct", "loguniform")))
    assert is_channel(ep.dr_mass[DR_MASS_PLATE], "direct", "loguniform", interval, 1.0, 4.0)


def test_plate_density_parses_on_startup():
    t = task_of(MANI, plate(density=entry("on_startup", [0.5, 2.0]), mass=entry("on_reset", [-0.2, 0.2], "additive")))
    (ep,) = t.engine_params()
    assert is_channel(ep.dr_mass[DR_MASS_PLATE_DENSITY], "scaling", "uniform", DR_ON_STARTUP, 0.5, 2.0)
    assert is_channel(ep.dr_mass[DR_MASS_PLATE], "additive", "uniform", 0, -0.2, 0.2)
    act = t._dr_randomizer.active_domain_randomizations
    assert ("rigid_prim_views", "plate", "density", "on_startup") in act and ("rigid_prim_views", "plate", "mass", "on_reset") in act


def test_body_masses_scalar_parameters():
    t = task_of(LOCO, robot(entry("on_interval", [0.5, 2.0], interval=7)))
    (ep,) = t.engine_params()
    assert ep.mode == MODE_LOCO
    assert is_channel(ep.dr_mass[DR_MASS_BODIES], "scaling", "uniform", 7, 0.5, 2.0)
    assert ep.dr_mass_body_p0 == [0.5] * 21 and ep.dr_mass_body_p1 == [2.0] * 21
    assert not ep.dr_mass[DR_MASS_PLATE].enabled and not ep.dr_mass[DR_MASS_PLATE_DENSITY].enabled
    assert ("articulation_views", "robot_view", "body_masses", "on_interval") in t._dr_randomizer.active_domain_randomizations
    md = lmlib.make_mass_dr(ep)
    assert md.ch[DR_MASS_BODIES].enabled == 1 and md.ch[DR_MASS_BODIES].interval == 7 and md.ch[DR_MASS_PLATE].enabled == 0
    assert list(md.body_p0) == [0.5] * 21 and list(md.body_p1) == [2.0] * 21
    assert lmlib.make_params(ep).dr_enabled == 1          # the parameter block itself does not carry them
    from oracle import lmo
    assert lmo.make_params(ep).dr_enabled == 1            # the oracle's make_params works on a block that carries the fields


@pytest.mark.parametrize("name,asset", [(LOCO, "quadruped_robot_v2"), (VERT, "quadfinger")])
def test_per_body_parameters_go_to_table_order(name, asset):
    """A (2, 21) block in body_names order with 21 different pairs: the engine's arrays are its table_body_order() permutation."""
    from locomanipulationrl_amd.model.robot_model import LIMB_BODIES, load_model
    rm = load_model(asset)
    order = rm.table_body_order()
    assert sorted(order) == list(range(21)) and order[0] == 0
    assert order[1:] == [int(k) for k in np.asarray(rm.limb_body_index).ravel()] and rm.limb_body_index.shape == (4, len(LIMB_BODIES))
    lo = [0.5 + 0.01 * k for k in range(21)]; hi = [1.5 + 0.02 * k for k in range(21)]
    (ep,) = blocks(name, robot(entry("on_startup", [lo, hi])))
    assert ep.dr_mass[DR_MASS_BODIES].enabled == 1 and ep.dr_mass[DR_MASS_BODIES].interval == DR_ON_STARTUP
    assert ep.dr_mass_body_p0 == [lo[k] for k in order] and ep.dr_mass_body_p1 == [hi[k] for k in order]
    md = lmlib.make_mass_dr(ep)
    assert np.allclose(list(md.body_p0), [lo[k] for k in order], atol=1e-7) and np.allclose(list(md.body_p1), [hi[k] for k in order], atol=1e-7)
    # the packed table carries the masses in the same order (slot s of the table = body order[s])
    tab = rm.packed_table()
    for limb in range(4):
        for j in range(5):
            assert tab[10 + 123 * limb + 65 + 10 * j] == np.float32(rm.mass[order[1 + 5 * limb + j]])
    assert tab[0] == np.float32(rm.mass[order[0]])


def test_cotraining_scopes_the_plate_channels():
    prm = {**robot(entry("on_startup", [0.5, 2.0])), **plate(mass=entry("on_interval", [0.5, 2.0]), density=entry("on_startup", [0.8, 1.2]))}
    lo, ma = blocks(BOTH, prm)
    assert (lo.mode, ma.mode) == (MODE_LOCO, MODE_MANI)
    assert not lo.dr_mass[DR_MASS_PLATE].enabled and not lo.dr_mass[DR_MASS_PLATE_DENSITY].enabled
    assert is_channel(ma.dr_mass[DR_MASS_PLATE], "scaling", "uniform", 3, 0.5, 2.0)
    assert is_channel(ma.dr_mass[DR_MASS_PLATE_DENSITY], "scaling", "uniform", DR_ON_STARTUP, 0.8, 1.2)
    for ep in (lo, ma):
        assert is_channel(ep.dr_mass[DR_MASS_BODIES], "scaling", "uniform", DR_ON_STARTUP, 0.5, 2.0)
        assert ep.dr_mass_body_p0 == [0.5] * 21


NAN = float("nan")
REFUSALS = [
    # (task, randomization_params, exception, text the message must carry)
    (LOCO, robot({**entry("on_reset", [0.5, 2.0]), **entry("on_interval", [0.5, 2.0])}), NotImplementedError, "body_masses"),          # two triggers
    (MANI, plate(mass={**entry("on_startup", [0.5, 2.0]), **entry("on_reset", [0.5, 2.0])}), NotImplementedError, "plate.mass"),
    (MANI, plate(density=entry("on_reset", [0.5, 2.0])), NotImplementedError, "no volume"),
    (MANI, plate(density=entry("on_interval", [0.5, 2.0])), NotImplementedError, "no volume"),
    (MANI, plate(density=entry("on_startup", [0.0, 0.1], "additive")), ValueError, "no volume"),
    (MANI, plate(density=entry("on_startup", [900.0, 1100.0], "direct")), ValueError, "no volume"),
    (LOCO, plate(mass=entry("on_reset", [0.5, 2.0])), NotImplementedError, "mass"),          # no plate in a locomotion task
    (LOCO, plate(mass=entry("on_startup", [0.5, 2.0])), NotImplementedError, "mass"),
    (LOCO, plate(density=entry("on_startup", [0.5, 2.0])), NotImplementedError, "density"),
    (LOCO, {"rigid_prim_views": {"baselink_view": {"mass": entry("on_startup", [0.9, 1.1])}}}, NotImplementedError, "body_masses"),      # base link: component 0
    (LOCO, {"rigid_prim_views": {"baselink_view": {"mass": entry("on_reset", [0.9, 1.1])}}}, NotImplementedError, "body_masses"),
    (MANI, {"rigid_prim_views": {"baselink_view": {"density": entry("on_startup", [0.9, 1.1])}}}, NotImplementedError, "body_masses"),
    (LOCO, robot(entry("on_reset", [0.0, 2.0])), ValueError, "non-positive"),                          # scaling by U(0, 2) reaches 0
    (LOCO, robot(entry("on_reset", [-1.0, 1.0], "additive")), ValueError, "non-positive"),             # the lightest link weighs far less than 1 kg
    (LOCO, robot(entry("on_reset", [-0.1, 0.3], "direct")), ValueError, "non-positive"),
    (MANI, plate(mass=entry("on_reset", [-2.4, 1.0], "additive")), ValueError, "non-positive"),        # 2.4 kg - 2.4 kg
    (MANI, plate(mass=entry("on_reset", [-1.3, 1.0], "additive"), density=entry("on_startup", [0.5, 2.0])), ValueError, "non-positive"),      # 0.5 x 2.4 - 1.3
    (MANI, plate(density=entry("on_startup", [-0.5, 2.0])), ValueError, "non-positive"),
    (LOCO, robot(entry("on_reset", [0.5, NAN])), ValueError, "finite"),
    (MANI, plate(mass=entry("on_reset", [float("inf"), 1.0], "additive", "gaussian")), ValueError, "finite"),
    (LOCO, robot(entry("on_reset", [0.0, 2.0], dist="loguniform")), ValueError, "loguniform"),
    (MANI, plate(mass=entry("on_reset", [-1.0, 2.0], dist="loguniform")), ValueError, "loguniform"),
    (LOCO, robot(entry("on_reset", [[0.5] * 20, [2.0] * 20])), ValueError, "21"),                      # a (2, 20) block
    (MANI, plate(mass=entry("on_reset", [[0.5] * 21, [2.0] * 21])), ValueError, "plate.mass"),         # the plate is one body
    (LOCO, robot(entry("on_interval", [0.5, 2.0], interval=0)), ValueError, "frequency_interval"),
    (LOCO, robot({"on_interval": dict(operation="scaling", distribution="uniform", distribution_parameters=[0.5, 2.0])}), ValueError, "frequency_interval"),
    (LOCO, robot(entry("on_reset", [0.5, 2.0], op="multiply")), ValueError, "body_masses"),
    (LOCO, robot(None), ValueError, "body_masses"),
    (LOCO, {"articulation_views": {"robot_view": {"body_inertias": entry("on_reset", [0.5, 2.0])}}}, NotImplementedError, "body_inertias"),
    (LOCO, {"articulation_views": {"robot_view": {"stiffness": entry("on_reset", [0.5, 2.0])}}}, NotImplementedError, "stiffness"),
    (MANI, plate(restitution=entry("on_reset", [0.5, 2.0])), NotImplementedError, "restitution"),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_refusals_name_the_reason(case):
    name, prm, exc, text = REFUSALS[case]
    with pytest.raises(exc) as ei:
        blocks(name, prm)
    assert text in str(ei.value), str(ei.value)


def test_a_positive_bounded_range_and_a_gaussian_are_accepted():
    (ep,) = blocks(LOCO, robot(entry("on_reset", [-0.001, 0.05], "additive")))          # the lightest link stays positive
    assert ep.dr_mass[DR_MASS_BODIES].enabled
    (ep,) = blocks(LOCO, robot(entry("on_reset", [0.0, 5.0], "additive", "gaussian")))  # a wide gaussian: the floor's business
    assert ep.dr_mass[DR_MASS_BODIES].enabled and DR_MASS_FLOOR == 0.05


def test_mass_struct_matches_the_header():
    """lm_mass_dr is three lm_dr_channel and two float[21]; lm_params, the ABI number and LM_DR_PHYS_ROWS are what they were."""
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "lm_engine.h"\nint main(){printf("%zu %zu %zu %d %d %d %d %d %d %zu %f %d %d %d\\n", sizeof(lm_mass_dr), '
           'offsetof(lm_mass_dr, body_p0), offsetof(lm_mass_dr, body_p1), LM_DR_MASS_CHANNELS, LM_DR_MASS_ROWS, (int)LM_PTR_DR_MASS, LM_NUM_BODIES, '
           'LM_ABI_VERSION, LM_DR_PHYS_ROWS, sizeof(lm_params), (double)LM_DR_MASS_FLOOR, LM_DR_MASS_PLATE, LM_DR_MASS_PLATE_DENSITY, LM_DR_MASS_BODIES);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c"); open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = subprocess.check_output([exe]).split()
    size, off0, off1, nch, rows, kind, nb, abi, phys_rows, psize = map(int, out[:10])
    floor = float(out[10]); enums = tuple(map(int, out[11:]))
    M = lmlib.LmMassDr
    assert (size, off0, off1) == (C.sizeof(M), M.body_p0.offset, M.body_p1.offset) == (3 * C.sizeof(lmlib.LmDrChannel) + 2 * 21 * 4, 3 * C.sizeof(lmlib.LmDrChannel),
                                                                                      3 * C.sizeof(lmlib.LmDrChannel) + 21 * 4)
    assert (nch, rows, kind, nb) == (lmlib.DR_MASS_CHANNELS, lmlib.DR_MASS_ROWS, lmlib.PTR_DR_MASS, lmlib.NUM_BODIES) == (3, 23, 11, 21)
    assert DR_MASS_ROWS == 23 and DR_MASS_CHANNELS == 3
    assert (abi, phys_rows, psize) == (5, 43, C.sizeof(lmlib.LmParams)) and lmlib.ABI_VERSION == 5 and lmlib.DR_PHYS_ROWS == 43
    assert abs(floor - DR_MASS_FLOOR) < 1e-9
    assert enums == (DR_MASS_PLATE, DR_MASS_PLATE_DENSITY, DR_MASS_BODIES) == (0, 1, 2)


def test_without_the_entries_no_mass_channel_is_on():
    """Every shipped task, randomisation on and off: dr_mass is all off, and so is the C struct made from it."""
    for name in TASKS:
        for dr in (False, True):
            for ep in blocks(name, None, randomize=dr):
                assert all_off(ep), (name, dr)
                assert not any(c.enabled for c in lmlib.make_mass_dr(ep).ch)
    assert all_off(EngineParams()) and all_off(loco_params(dr_enabled=1))
    assert not any(c.enabled for c in lmlib.make_mass_dr(loco_params()).ch)


def test_entry_point_refuses_null_arguments_without_a_gpu():
    """lm_set_mass_randomization needs a live handle for everything else (an engine exists only on a GPU): those refusals are in
    tests/test_gpu_mass_dr.py::test_entry_point_refusals."""
    so = lmlib.load_library() if os.path.exists(lmlib._SO) else (lmlib.build_library(), lmlib.load_library())[1]
    assert "lm_set_mass_randomization" in lmlib.EXPORTS
    md = lmlib.LmMassDr()
    assert so.lm_set_mass_randomization(None, 0, C.byref(md)) == -1 and b"lm_set_mass_randomization" in so.lm_last_error()


def test_plate_mass_range_is_checked_against_the_blocks_own_plate():
    """additive U(-1.2, 1) keeps the shipped 2.4 kg plate positive and is accepted; the same entry on a block built with a 1 kg plate is refused."""
    t = task_of(MANI, plate(mass=entry("on_reset", [-1.2, 1.0], "additive")))
    (ep,) = t.engine_params()
    assert ep.plate_mass == 2.4 and ep.dr_mass[DR_MASS_PLATE].enabled
    with pytest.raises(ValueError, match="non-positive"):
        t._common(t.robot_manipulation, mode=MODE_MANI, plate_mass=1.0)
    heavy = t._common(t.robot_manipulation, mode=MODE_MANI, plate_mass=5.0)
    assert heavy.plate_mass == 5.0 and heavy.dr_mass[DR_MASS_PLATE].enabled
