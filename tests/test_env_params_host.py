"""Per-env physics parameters held by the caller, the parts that need no GPU: the name -> row map of the hold table, the shape and
name errors of Engine.set_env_params' front end, the sweep grids of tools/eval_policy.py --sweep, EpisodeRecord.summary_by, and the C entry
points' argument validation."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from locomanipulationrl_amd import lib as lmlib
from locomanipulationrl_amd.train import evaluate as ev


def test_name_map_covers_the_69_rows_once_and_matches_the_records():
    assert lmlib.ENV_PARAM_ROWS == 69 == lmlib.DR_PHYS_ROWS + lmlib.DR_MASS_ROWS + lmlib.DR_ACTUATOR_ROWS
    rows = []
    for name in lmlib.ENV_PARAMS:
        r0, n = lmlib.env_param_rows(name)
        rows += list(range(r0, r0 + n))
    assert sorted(rows) == list(range(69))          # every row exactly once
    # LM_PTR_DR_PHYS: max efforts 12, max joint velocities 12, gravity 3, base force 3, joint damping 12, mu_env 1 (row LM_DR_PHYS_MU)
    assert [lmlib.env_param_rows(k) for k in ("max_efforts", "max_velocities", "gravity", "base_force", "joint_damping", "mu")] == \
        [(0, 12), (12, 12), (24, 3), (27, 3), (30, 12), (lmlib.DR_PHYS_MU, 1)]
    # LM_PTR_DR_MASS behind it: plate mass, plate inertia factor, 21 body masses; LM_PTR_DR_ACTUATOR behind that: kp, kd, latency
    m0, a0 = lmlib.DR_PHYS_ROWS, lmlib.DR_PHYS_ROWS + lmlib.DR_MASS_ROWS
    assert [lmlib.env_param_rows(k) for k in ("plate_mass", "plate_inertia_factor", "body_masses")] == [(m0, 1), (m0 + 1, 1), (m0 + 2, lmlib.NUM_BODIES)]
    assert [lmlib.env_param_rows(k) for k in ("kp", "kd", "latency")] == [(a0, 1), (a0 + 1, 1), (a0 + 2, 1)]
    # the header says the same
    hdr = open(os.path.join(ROOT, "include", "lm_engine.h")).read()
    assert re.search(r"#define LM_ENV_PARAM_ROWS \(LM_DR_PHYS_ROWS \+ LM_DR_MASS_ROWS \+ LM_DR_ACTUATOR_ROWS\)", hdr)
    assert int(re.search(r"LM_PTR_ENV_PARAMS = (\d+)", hdr).group(1)) == lmlib.PTR_ENV_PARAMS == 14
    assert int(re.search(r"#define LM_ABI_VERSION (\d+)", hdr).group(1)) == 5          # no ABI bump: lm_params is untouched


def test_shape_and_name_errors():
    N = 40
    assert lmlib.env_param_shape("mu", N) == (N,) and lmlib.env_param_shape("body_masses", N) == (21, N) and lmlib.env_param_shape("gravity", N) == (3, N)
    a = lmlib.env_param_values("mu", np.linspace(0.2, 1.2, N), N)
    assert a.shape == (1, N) and a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    assert np.array_equal(lmlib.env_param_values("kp", 3.0, N), np.full((1, N), 3.0, np.float32))          # a scalar holds every env
    b = lmlib.env_param_values("body_masses", np.arange(21 * N, dtype=np.float64).reshape(21, N), N)
    assert b.shape == (21, N) and b[3, 7] == 3 * N + 7
    import torch
    assert lmlib.env_param_values("gravity", torch.zeros(3, N), N).shape == (3, N)
    with pytest.raises(ValueError, match="unknown env parameter 'friction'"):
        lmlib.env_param_rows("friction")
    with pytest.raises(ValueError, match="unknown env parameter"):
        lmlib.env_param_values("masses", np.zeros(N), N)
    for name, bad in (("mu", np.zeros((1, N))), ("mu", np.zeros(N - 1)), ("body_masses", np.zeros((N, 21))), ("gravity", np.zeros(N)), ("max_efforts", np.zeros((3, N)))):
        with pytest.raises(ValueError, match="values of shape"):
            lmlib.env_param_values(name, bad, N)


def test_sweep_grids_parse_and_assign():
    name, v = ev.parse_sweep("mu=0.2:1.2:6")
    assert name == "mu" and np.allclose(v, np.linspace(0.2, 1.2, 6))
    assert np.array_equal(ev.parse_sweep("latency=0:3:3")[1], [0.0, 2.0, 3.0])          # whole sub-steps (1.5 rounds to even)
    assert np.array_equal(ev.parse_sweep("plate_mass=2:9:1")[1], [2.0])
    for bad in ("mu", "mu=1:2", "mu=a:b:3", "stiffness=1:2:3", "mu=0:1:0", "mu=0:inf:3", "mu=1:2:3=4"):
        with pytest.raises(ValueError):
            ev.parse_sweep(bad)
    sw = [ev.parse_sweep("mu=0.4:1.0:4"), ev.parse_sweep("base_mass_add=0:0.3:2"), ev.parse_sweep("kp_scale=0.5:2:3")]
    pts = ev.sweep_grid(sw)
    assert len(pts) == 24 and pts[0] == {"mu": 0.4, "base_mass_add": 0.0, "kp_scale": 0.5} and pts[1]["kp_scale"] == 1.25 and pts[3]["base_mass_add"] == 0.3
    assert len({tuple(sorted(p.items())) for p in pts}) == 24          # the whole product, every point once
    with pytest.raises(ValueError):
        ev.sweep_grid([sw[0], sw[0]])
    N = 64
    g = ev.sweep_groups(N, 24)
    assert g.dtype == np.int64 and np.array_equal(g, np.arange(N) % 24)          # env e gets grid point e % K_total
    assert set(g[:32].tolist()) == set(range(24)) == set(g[32:].tolist() + g[:32].tolist())
    with pytest.raises(ValueError):
        ev.sweep_groups(16, 24)
    # the held values of the grid: absolute names as given, relative ones on the nominal values handed in
    m = np.linspace(0.1, 2.1, 21); kp = np.where(np.arange(N) < 32, 5.0, 8.0); kd = np.full(N, 0.5)
    held = ev.sweep_env_params(pts, g, body_masses=m, kp=kp, kd=kd)
    assert sorted(held) == ["body_masses", "kp", "mu"] and all(v.dtype == np.float32 for v in held.values())
    for e in (0, 5, 23, 24, 63):
        p = pts[e % 24]
        assert held["mu"][e] == np.float32(p["mu"]) and held["kp"][e] == np.float32(kp[e] * p["kp_scale"])
        assert held["body_masses"][0, e] == np.float32(m[0] + p["base_mass_add"]) and np.array_equal(held["body_masses"][1:, e], m[1:].astype(np.float32))
    for k, v in held.items():
        assert v.shape == lmlib.env_param_shape(k, N)
    h2 = ev.sweep_env_params(ev.sweep_grid([ev.parse_sweep("body_mass_scale=0.5:2:4"), ev.parse_sweep("max_effort=0.5:1.5:2"), ev.parse_sweep("kd_scale=1:2:2")]),
                             ev.sweep_groups(N, 16), body_masses=m, kp=kp, kd=kd)
    assert sorted(h2) == ["body_masses", "kd", "max_efforts"] and h2["max_efforts"].shape == (12, N) and (h2["max_efforts"][:, 2] == 1.5).all()
    assert np.allclose(h2["body_masses"][:, 4], m * 1.0) and np.allclose(h2["body_masses"][:, 63], m * 2.0) and h2["kd"][1] == 1.0 and h2["kd"][2] == 0.5


def test_summary_by_equals_reduce_per_group():
    rng = np.random.default_rng(0)
    N = 50
    rec = np.zeros((lmlib.EPISODE_ROWS, N))
    rec[2] = rng.integers(0, 4, N); rec[3] = rng.normal(size=N) * rec[2]; rec[4] = rng.integers(1, 90, N) * rec[2]
    rec[5] = rng.integers(0, 2, N) * (rec[2] > 0); rec[6] = np.minimum(rec[2] - rec[5], rng.integers(0, 2, N)); rec[7] = rec[2] - rec[5] - rec[6]
    groups = np.arange(N) % 4
    groups[groups == 3] = 7          # ids need not be dense
    by = lmlib.EpisodeRecord.reduce_by(rec, groups)
    assert list(by) == [0, 1, 2, 7]
    for k in by:
        assert by[k] == lmlib.EpisodeRecord._reduce(rec[:, groups == k])
    assert sum(v["episodes"] for v in by.values()) == lmlib.EpisodeRecord._reduce(rec)["episodes"]
    import torch
    assert lmlib.EpisodeRecord.reduce_by(rec, torch.as_tensor(groups)) == by

    class _Rec:          # summary_by is reduce_by on the record of the instance
        record = torch.as_tensor(rec, dtype=torch.float32)
    assert lmlib.EpisodeRecord.summary_by(_Rec(), groups) == lmlib.EpisodeRecord.reduce_by(_Rec.record.double().numpy(), groups)
    with pytest.raises(ValueError):
        lmlib.EpisodeRecord.reduce_by(rec, np.arange(N - 1))
    with pytest.raises(ValueError):
        lmlib.EpisodeRecord.reduce_by(rec, np.zeros(N))          # float ids


def test_entry_points_refuse_a_null_handle_without_gpu():
    lmlib.build_library()
    so = lmlib.load_library()
    for n in ("lm_enable_env_params", "lm_set_env_params", "lm_clear_env_params", "lm_env_params_held"):
        assert n in lmlib.EXPORTS and hasattr(so, n)
    v = (C.c_float * 4)()
    m = (C.c_uint64 * 2)()
    assert so.lm_enable_env_params(None) == -1 and b"lm_enable_env_params" in so.lm_last_error() and b"null" in so.lm_last_error()
    assert so.lm_set_env_params(None, 0, 1, C.cast(v, C.c_void_p)) == -1 and b"lm_set_env_params" in so.lm_last_error()
    assert so.lm_clear_env_params(None, 0, 1) == -1 and b"lm_clear_env_params" in so.lm_last_error()
    assert so.lm_env_params_held(None, m) == -1 and b"lm_env_params_held" in so.lm_last_error()
    assert so.lm_ptr(None, lmlib.PTR_ENV_PARAMS) is None
