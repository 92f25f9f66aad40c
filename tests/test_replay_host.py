"""Replay of recorded joint motions, host side (no GPU): the float64 reference of the rule (tests/replay_reference.py, written from
include/lm_policy.h) against the helper the project's evidence was produced with (npy_replay.replay) on its own per-step stream; the torch
path of lib.ReplayRecord on the CPU oracle backend against that reference; the env layout and the refusals of train.replay.replay_sweep; its
leave-one-out reduction; the header's constants and the device-free LM_EINVAL cases; and what the fp32 oracle gives through the whole Python
path (the thresholds the GPU tests assert)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import npy_replay as R
import replay_reference as ref
import test_reference_npy_replay as T
from conftest import ROOT
from locomanipulationrl_amd import lib as lmlib
from locomanipulationrl_amd.engine_config import loco_cc_params, loco_params, mani_params
from locomanipulationrl_amd.lib import ReplayPlan, ReplayRecord
from locomanipulationrl_amd.train import replay as RP
from oracle_backend import OracleEngine

V2_THRESH = np.sin(0.075) ** 2


@pytest.fixture(scope="module")
def recordings():
    return R.load()


def logged(step):
    log = []

    def f(a):
        out = step(a)
        log.append((np.asarray(a, dtype=np.float64).copy(),) + tuple(out))
        return out
    return f, log


# ---------------------------------------------------------------------------------------------------------------- reference == replay()
@pytest.mark.parametrize("servo, hold", [(False, 0), (False, 2), (True, 0)])
def test_reference_reproduces_npy_replay(robot_model, recordings, servo, hold):
    """Fed the (q, obs, flags, reward) stream of npy_replay.replay() on the fp64 oracle, the reference reproduces replay()'s outputs and the
    actions replay() fed: integers exactly, floats to 1e-12."""
    for name in R.FILES:
        rec = recordings[name]; L = len(rec)
        step, log = logged(R.oracle_stepper(robot_model, R.cotrain_params(R.kind_of(name))))
        out = R.replay(rec, step, servo=servo, until_done=hold > 0)
        act = np.concatenate([np.zeros((1, 12)), R.recovered_actions(rec)])
        plan = ref.Plan(rec[None], act[None], [L], [0], servo, hold, 17, 1.0 / R.FULL, V2_THRESH, 1e-3)
        record = ref.zero_record(1); nxt = np.zeros((1, 12))
        assert log[0][3] == 0, name                            # no reset flag on row 0: the one stated difference never shows
        for s, (a, q, obs, rst, goal, rew) in enumerate(log):
            assert np.abs(a - nxt[0]).max() <= 1e-12, (name, s)          # the reference's actions_next are the actions replay() applied
            nxt = ref.update(plan, record, s, q[:, None], obs[None], [rew], [goal], [rst])
        assert record[ref.FINISHED, 0] == 1 or len(log) == L + hold, name          # replay() stopped where the rule stops
        assert np.abs(nxt).max() == 0.0
        s = {k: v[0] for k, v in ref.summary(record, R.FULL).items()}
        n = len(out["rows"])
        assert s["rows"] == n and s["done_at"] == (-1 if out["done_at"] is None else out["done_at"]) and s["goal"] == out["goal"], name
        assert s["first_succ"] == (-1 if out["first_succ"] is None else out["first_succ"]) and s["in_window"] == out["in_window"], name
        err = out["rows"] - rec[:n]
        want = dict(row0_err=out["row0_err"], qerr=out["qerr"], tracked=out["tracked"], early=out["early"], min_rd=out["rd_rec"].min(), rd_first=out["rd"][0],
                    rms=np.sqrt((err ** 2).mean()), mean_abs=np.abs(err).mean(), window_return=out["rew"][L - 17:L].sum())
        want["return"] = out["rew"].sum()
        for k, v in want.items():
            assert abs(s[k] - v) <= 1e-12 * max(1.0, abs(v)), (name, k, s[k], v)
        assert np.abs(record[ref.QPREV:ref.QPREV + 12, 0] - out["rows"][-1]).max() == 0.0


# ---------------------------------------------------------------------------------------------------------------- torch path == reference
LOCO3 = ["mlp_joint_loco", "mlp_loco_from_mani", "test"]
MANI3 = ["mlp_joint_mani", "mlp_mani_from_loco", "04roll_mani_from_scratch"]


def cotrain_engine(robot_model, n_half=16, precision="f64"):
    return OracleEngine(robot_model, [R.cotrain_params("loco"), R.cotrain_params("mani")], 2 * n_half, n_half, 0, 5.0, 1.0, precision=precision)


def run_both(eng, plan, check_actions=None):
    """plan.run() by hand with the reference alongside: returns (ReplayRecord, reference record, smallest threshold margins)."""
    N = eng.num_envs
    rp = ref.Plan(plan.rec_t.numpy(), plan.act_t.numpy(), plan.len_t.numpy(), plan.env_rec_t.numpy(), plan.servo, plan.hold, plan.window_rows, plan.inv_full,
                  plan.v2_thresh, plan.track_tol)
    assert rp.steps() == plan.steps
    record = ReplayRecord(eng); want = ref.zero_record(N)
    actions = torch.zeros(N, 12); obs = torch.empty(N, 64); rew = torch.empty(N)
    mt, mv = np.inf, np.inf
    for s in range(plan.steps):
        eng.step(actions, out_obs=obs, out_rew=rew)
        q, cnt = eng.state[13:25].numpy(), eng.cnt.numpy()
        a, b = ref.margins(rp, want, s, q, obs.numpy()); mt, mv = min(mt, a), min(mv, b)
        nxt = ref.update(rp, want, s, q, obs.numpy(), rew.numpy(), cnt[2], cnt[3])
        record.update(plan, s, obs, rew, actions)
        if plan.servo:
            assert np.abs(actions.numpy() - nxt).max() <= 2e-6, s          # fp32 against fp64 of a value within +-1 (a few ulp of the difference x 10)
        else:
            assert np.array_equal(actions.numpy(), nxt.astype(np.float32)), s          # a copy of the table
    return record, want, (mt, mv)


def assert_records_match(got, want, part):
    got = got.double().numpy()
    for r in ref.INTEGER_ROWS:
        assert np.array_equal(got[r, part], want[r, part]), (r, got[r, part], want[r, part])
    for r in ref.FLOAT_ROWS:
        a, b = got[r, part], want[r, part]
        assert np.array_equal(np.isinf(a), np.isinf(b)) and (np.abs(a - b)[np.isfinite(b)] <= 1e-5 * np.maximum(np.abs(b[np.isfinite(b)]), 1e-3)).all(), (r, a, b)


@pytest.mark.parametrize("servo", [False, True])
def test_torch_path_equals_reference(robot_model, recordings, servo):
    """ReplayRecord's torch path on the oracle backend (16 + 16 co-training envs, three files per half, the rest taking no part) against the
    reference on the same stream: integer rows exactly, float rows to 1e-5, the columns of the envs that take no part as zero() left them."""
    eng = cotrain_engine(robot_model)
    names = LOCO3 + MANI3
    env_rec = np.full(32, -1, dtype=np.int32); env_rec[[0, 1, 2, 5]] = [0, 1, 2, 0]; env_rec[[16, 17, 18, 31]] = [3, 4, 5, 4]
    plan = ReplayPlan(eng, [recordings[n] for n in names], env_rec, servo=servo, hold=2)
    assert plan.full == R.cotrain_params("loco").act_scale * R.cotrain_params("loco").ctrl_dt and abs(plan.full - R.FULL) < 1e-15
    record, want, (mt, mv) = run_both(eng, plan)
    print("threshold margins: track_tol", mt, "v2_thresh", mv)
    assert mt > 1e-6 and mv > 1e-6          # the fp32 path decides every comparison as fp64 does: the fp32 error of the compared values is ~1e-7
    part = env_rec >= 0
    assert_records_match(record.record, want, part)
    blank = ReplayRecord(eng).record
    assert torch.equal(record.record[:, ~torch.from_numpy(part)], blank[:, ~torch.from_numpy(part)])
    assert (record.record[28:] == 0).all()
    assert np.array_equal(record.record[:, 0].numpy(), record.record[:, 5].numpy())          # the same recording on the same block: the same bits
    s = record.summary(); w = ref.summary(want, plan.full)
    for k in w:
        a, b = np.asarray(s[k], dtype=np.float64)[part], np.asarray(w[k], dtype=np.float64)[part]
        assert np.allclose(a, b, rtol=2e-5, atol=1e-7, equal_nan=True), (k, a, b)
    # plan.run() is that loop
    eng2 = cotrain_engine(robot_model)
    plan2 = ReplayPlan(eng2, [recordings[n] for n in names], env_rec, servo=servo, hold=2)
    again = plan2.run(ReplayRecord(eng2))
    assert torch.equal(again.record, record.record)


def test_default_action_table_and_argument_errors(robot_model, recordings):
    eng = cotrain_engine(robot_model)
    rec = recordings["test"]; env_rec = np.full(32, -1, dtype=np.int32); env_rec[3] = 0
    plan = ReplayPlan(eng, [rec], env_rec)
    assert plan.steps == len(rec) + 2 and plan.T_max == len(rec) and plan.R == 1
    want = np.concatenate([np.zeros((1, 12)), R.recovered_actions(rec)]).astype(np.float32)          # what recovered_actions feeds today
    assert np.array_equal(plan.act_t[0].numpy(), want) and np.array_equal(plan.rec_t[0].numpy(), rec.astype(np.float32))
    assert plan.inv_full == float(np.float32(1.0 / plan.full)) and plan.v2_thresh == float(np.float32(V2_THRESH))
    assert ReplayPlan(eng, [rec], np.full(32, -1, dtype=np.int32)).steps == 0
    for bad in (dict(recordings=[]), dict(recordings=[rec[:, :11]]), dict(env_rec=env_rec[:31]), dict(env_rec=env_rec.astype(np.float64)), dict(actions=[rec[:-1]]),
                dict(hold=9), dict(hold=-1), dict(window_rows=len(rec) + 1), dict(env_rec=np.where(env_rec >= 0, 1, -1).astype(np.int32)),
                dict(env_rec=np.full(32, -2, dtype=np.int32)), dict(recordings=[np.where(np.arange(len(rec))[:, None] == 4, np.nan, rec)])):
        with pytest.raises(ValueError):
            ReplayPlan(**{**dict(engine=eng, recordings=[rec], env_rec=env_rec), **bad})
    other = OracleEngine(robot_model, [R.cotrain_params("loco"), R.cotrain_params("mani", act_scale=2.0)], 32, 16, 0, 5.0, 1.0)
    with pytest.raises(ValueError, match="act_scale"):
        ReplayPlan(other, [rec], env_rec)
    for make in (loco_cc_params, lambda: loco_params(drive_mode=1)):          # what the library refuses, the torch path refuses too
        pd = OracleEngine(robot_model, [make()], 32, None, 0, 5.0, 1.0)
        with pytest.raises(ValueError, match="variant 0 in velocity drive"):
            ReplayPlan(pd, [rec], env_rec)


# ---------------------------------------------------------------------------------------------------------------- layout, refusals, leave-one-out
def test_layout_pads_each_half_to_16_and_refuses_what_does_not_fit():
    kinds = {n: R.kind_of(n) for n in R.FILES}
    lay = RP.replay_layout(R.FILES, kinds, [0, 1], 2)
    assert lay["num_envs"] == 32 and lay["split"] == 16          # 7 x 2 -> 16, 4 x 2 -> 16
    loco = [n for n in R.FILES if kinds[n] == "loco"]; mani = [n for n in R.FILES if kinds[n] == "mani"]
    assert len(loco) == 7 and len(mani) == 4
    for f, n in enumerate(loco):
        for p in range(2):
            e = lay["env_of"][(n, p)]
            assert e == 2 * f + p and lay["env_rec"][e] == R.FILES.index(n) and lay["groups"][e] == p
    for f, n in enumerate(mani):
        for p in range(2):
            e = lay["env_of"][(n, p)]
            assert e == 16 + 2 * f + p and lay["env_rec"][e] == R.FILES.index(n) and lay["groups"][e] == p
    assert (lay["env_rec"][14:16] == -1).all() and (lay["env_rec"][24:] == -1).all() and lay["env_rec"].dtype == np.int32
    big = RP.replay_layout(R.FILES, kinds, [0, 1], 13)
    assert (big["split"], big["num_envs"]) == (96, 160)          # 91 -> 96, 52 -> 64
    one = RP.replay_layout(loco, kinds, [0], 3)
    assert one["num_envs"] == 32 and one["split"] is None
    with pytest.raises(ValueError, match="no mani block"):
        RP.replay_layout(R.FILES, kinds, [0], 2)
    with pytest.raises(ValueError, match="no loco block"):
        RP.replay_layout(loco, {n: "loco" for n in loco}, [1], 2)
    with pytest.raises(ValueError, match="'loco' or 'mani'"):
        RP.replay_layout(loco, {**kinds, loco[0]: "arm"}, [0, 1], 2)
    with pytest.raises(ValueError, match="does not fit"):
        RP.replay_layout(R.FILES, kinds, [0, 1], 13, max_envs=128)
    with pytest.raises(ValueError, match="empty"):
        RP.replay_layout(R.FILES, kinds, [0, 1], 0)


def test_replay_sweep_refuses_before_it_creates_an_engine(robot_model, recordings):
    """A manipulation recording assigned to a locomotion block (and the other way round) and a grid that does not fit raise ValueError; no
    engine is made (none could be: there is no device here)."""
    def no_engine(*a, **k):
        raise AssertionError("an engine was created")
    recs = {n: recordings[n] for n in ("mlp_joint_loco", "mlp_joint_mani")}
    params = [R.cotrain_params("loco"), R.cotrain_params("mani")]
    with pytest.raises(ValueError, match="no mani block"):
        RP.replay_sweep(robot_model, params[:1], recs, {"mlp_joint_loco": "loco", "mlp_joint_mani": "mani"}, [{"mu": 0.8}], engine_cls=no_engine)
    with pytest.raises(ValueError, match="no loco block"):
        RP.replay_sweep(robot_model, params[1:], recs, {"mlp_joint_loco": "loco", "mlp_joint_mani": "mani"}, [{"mu": 0.8}], engine_cls=no_engine)
    with pytest.raises(ValueError, match="does not fit"):
        RP.replay_sweep(robot_model, params, recs, {"mlp_joint_loco": "loco", "mlp_joint_mani": "mani"}, [{"mu": m} for m in np.linspace(0.5, 1.2, 40)],
                        max_envs=64, engine_cls=no_engine)
    with pytest.raises(ValueError, match="score_files"):
        RP.replay_sweep(robot_model, params, recs, {"mlp_joint_loco": "loco", "mlp_joint_mani": "mani"}, [{"mu": 0.8}], score_files=["nope"], engine_cls=no_engine)


def test_leave_one_out_is_the_existing_reduction():
    rng = np.random.default_rng(3)
    tab = {mu: [int(x) for x in rng.integers(0, 18, len(R.GOAL_KNOWN))] for mu in T.MU_GRID}
    tab[0.6] = list(tab[0.8])                                    # a tie: the first of the grid wins in both
    assert RP.leave_one_out(tab, R.GOAL_KNOWN) == T.leave_one_out(tab)
    flat = {mu: [5] * len(R.GOAL_KNOWN) for mu in T.MU_GRID}
    assert RP.leave_one_out(flat, R.GOAL_KNOWN) == T.leave_one_out(flat) and RP.leave_one_out(flat, R.GOAL_KNOWN)[0][1] == T.MU_GRID[0]


# ---------------------------------------------------------------------------------------------------------------- ABI
REPLAY_SYMBOLS = ("lm_replay_create", "lm_replay_steps", "lm_replay_update", "lm_replay_destroy")


def test_abi_of_the_replay_entry_points():
    lmlib.build_library()
    so = lmlib.load_library()
    for n in REPLAY_SYMBOLS:
        assert n in lmlib.EXPORTS and hasattr(so, n), n
    src = '#include <stdio.h>\n#include "lm_engine.h"\n#include "lm_policy.h"\nint main(){printf("%d %d %zu\\n", LM_REPLAY_ROWS, LM_ABI_VERSION, sizeof(lm_params));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c"); open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", os.path.join(d, "s")])
        rows, abi, size = map(int, subprocess.check_output([os.path.join(d, "s")]).split())
    assert rows == lmlib.REPLAY_ROWS == 32 == ref.ROWS
    assert abi == lmlib.ABI_VERSION == so.lm_abi_version() == 5          # the feature changes neither the version ...
    assert size == C.sizeof(lmlib.LmParams) == PARAMS_SIZE               # ... nor the parameter block
    assert max(lmlib.REPLAY.values()) + 12 <= lmlib.REPLAY_ROWS and lmlib.REPLAY["qprev"] == ref.QPREV
    # null arguments are refused before any device is touched
    h = C.c_void_p(); one = (C.c_float * 12)(); ids = (C.c_int32 * 1)(0)
    assert so.lm_replay_create(None, None, None, None, None, 1, 1, None, 0, 0, 1, 1.0, 1.0, 1.0) == -1 and b"null" in so.lm_last_error()
    assert so.lm_replay_create(C.byref(h), None, one, one, ids, 1, 1, ids, 0, 0, 1, 1.0, 1.0, 1.0) == -1 and b"null" in so.lm_last_error() and not h
    assert so.lm_replay_update(None, 0, None, None, None, None, None) == -1 and b"null" in so.lm_last_error()
    assert so.lm_replay_steps(None) == -1 and so.lm_replay_destroy(None) == 0


PARAMS_SIZE = 1404         # sizeof(lm_params) at LM_ABI_VERSION 5


# ---------------------------------------------------------------------------------------------------------------- CPU pre-check of the GPU thresholds
def fp32_runs(robot_model, recordings, servo):
    """All 11 files through the whole Python path on the fp32 oracle: one co-training engine, 7 + 4 files padded to 16 + 16."""
    kinds = {n: R.kind_of(n) for n in R.FILES}
    lay = RP.replay_layout(R.FILES, kinds, [0, 1], 1)
    eng = cotrain_engine(robot_model, precision="f32")
    plan = ReplayPlan(eng, [recordings[n] for n in R.FILES], lay["env_rec"], servo=servo, hold=0 if servo else 2)
    s = plan.run(ReplayRecord(eng)).summary()
    return {n: RP.as_replay_run({k: v[lay["env_of"][(n, 0)]] for k, v in s.items()}, len(recordings[n])) for n in R.FILES}


def test_fp32_oracle_servo_replays_stay_on_the_recording(robot_model, recordings):
    """The thresholds of test_servo_replay_keeps_the_joints_on_the_recording hold in fp32 (worst values measured: qerr 0.038, mean |error| 1.3e-3)."""
    runs = fp32_runs(robot_model, recordings, servo=True)
    print({n: (round(r["qerr"], 4), round(r["mean_abs"], 5)) for n, r in runs.items()})
    for n, r in runs.items():
        assert r["qerr"] <= 0.05 and r["mean_abs"] < 2e-3, (n, r["qerr"], r["mean_abs"])


def test_fp32_oracle_open_loop_replays_pass_the_orientation_checks(robot_model, recordings):
    runs = fp32_runs(robot_model, recordings, servo=False)
    print("shared window rows:", sum(runs[n]["in_window"] for n in R.GOAL_KNOWN))
    T.check_drive_limit(runs)
    T.check_orientation(runs)
