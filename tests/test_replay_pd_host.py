"""Replay of recorded commands on the PD-actuator tasks, host side (no GPU): the PD branch of lib.ReplayRecord's torch path against the float32
reference of the rule (tests/replay_pd_reference.py, written from include/lm_policy.h) bit for bit on synthetic state for the three engine
families and a co-training pair; the plan's refusals and keyword rules; the device-free refusals of lm_replay_create_pd; and on the CPU oracle a
walk recorded under random actions and replayed from its action log (exactly) and from its target log (to the rounding of the target map)."""
import ctypes as C

import numpy as np
import pytest
import torch

import replay_pd_reference as ref
from locomanipulationrl_amd import lib as lmlib
from locomanipulationrl_amd.engine_config import loco_cc_params, loco_params, loco_pc_params, mani_cc_params
from locomanipulationrl_amd.lib import ReplayPlan, ReplayRecord
from oracle_backend import OracleEngine

V2_THRESH = float(np.float32(np.sin(0.075) ** 2))
LENS, WINDOW, HOLD, TOL = (5, 21, 26), 4, 2, 1e-3

FAMILIES = {
    "cc": lambda: ([loco_cc_params()], None),                                                        # variant 1, 88-wide observations
    "pc": lambda: ([loco_pc_params()], None),                                                        # variant 2
    "pos": lambda: ([loco_params(drive_mode=1, act_scale=3.14159)], None),                           # variant 0 in position drive
    "cotrain": lambda: ([loco_cc_params(), mani_cc_params(act_scale_se=0.07)], 16),                  # two blocks, two reciprocals
}


def block_of(params, split, N):
    return [params[1 if (split and e >= split) else 0] for e in range(N)]


def synthetic_case(params, split, N, cmd_mode, seed=5):
    """Three recordings with their command tables, the env map, and per step what lm_step would have left: q and se (12, N), obs (N, width),
    rewards, goal and reset flags.  In targets mode the targets are spread far beyond [se_lo, se_hi], most of them further from the held command
    than act_scale_se (saturation) and some within it; the held command `se` is drawn anew every step, as a step would have clamped it.
    Envs 0 .. 5: finished on row 0 | on the last row | never | s + 1 == T reached without a flag (the 5-row recording) | on a hold row | idle."""
    rng = np.random.default_rng(seed)
    width = int(params[0].num_obs)
    recs = [np.cumsum(rng.uniform(-0.08, 0.08, (L, 12)), axis=0) + rng.uniform(-1.0, 1.0, 12) for L in LENS]
    if cmd_mode == ref.CMD_ACTIONS:
        cmds = [rng.uniform(-1.0, 1.0, a.shape) for a in recs]
    else:
        cmds = [rng.uniform(-4.0, 4.0, a.shape) for a in recs]
    env_rec = rng.integers(0, 3, N).astype(np.int32)
    env_rec[:6] = [1, 1, 2, 0, 1, -1]; env_rec[[N // 2, N - 1]] = -1
    T_of = np.array([LENS[r] if r >= 0 else 0 for r in env_rec])
    done_at = np.where(rng.random(N) < 0.5, rng.integers(1, np.maximum(T_of, 2)), -1)
    done_at[:6] = [0, 20, -1, -1, 21, -1]
    steps = max(LENS) + HOLD + 1
    blocks = block_of(params, split, N)
    lo = np.array([b.se_lo for b in blocks]).T; hi = np.array([b.se_hi for b in blocks]).T          # (12, N)
    stream = []
    for s in range(steps):
        q = np.stack([recs[max(r, 0)][min(s, max(T_of[e] - 1, 0))] for e, r in enumerate(env_rec)], axis=1) + rng.uniform(-5e-3, 5e-3, (12, N))
        se = rng.uniform(lo, hi)
        if cmd_mode == ref.CMD_TARGETS:          # a third of the envs hold a command within reach of the next logged one: unsaturated actions
            near = rng.random(N) < 0.33
            for e in np.nonzero(near & (env_rec >= 0))[0]:
                k = min(s + 1, T_of[e] - 1)
                c = ref.se_command(cmds[env_rec[e]][k]) if blocks[e].variant >= 1 else np.zeros(12)
                se[:, e] = c + rng.uniform(-0.06, 0.06, 12)
        obs = rng.uniform(-5.0, 5.0, (N, width))
        v2 = np.where(rng.random(N) < min(1.0, s / 12.0), rng.uniform(0.0, 5.0e-3, N), rng.uniform(6.2e-3, 0.5, N))
        d = rng.normal(size=(N, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        obs[:, 7:10] = d * np.sqrt(v2)[:, None]
        rst = (done_at == s) | ((done_at >= 0) & (s > done_at) & (rng.random(N) < 0.3))
        stream.append((q.astype(np.float32), se.astype(np.float32), obs.astype(np.float32), rng.uniform(0.5, 3.0, N).astype(np.float32),
                       (rng.random(N) < 0.5).astype(np.int64), rst.astype(np.int64)))
    return recs, cmds, env_rec, stream


def reference_run(params, split, recs, cmds, env_rec, stream, cmd_mode):
    """The reference over the whole stream: (plan, record, [actions_next per step])."""
    N = len(env_rec); Tm = max(LENS)
    rec = np.zeros((3, Tm, 12), dtype=np.float32); cmd = np.zeros_like(rec)
    for k in range(3):
        rec[k, :LENS[k]] = recs[k]; cmd[k, :LENS[k]] = cmds[k]
    blocks = block_of(params, split, N)
    plan = ref.Plan(rec, cmd, LENS, env_rec, cmd_mode, HOLD, WINDOW, V2_THRESH, np.float32(TOL), [b.variant for b in blocks],
                    [b.act_scale_se if b.variant >= 1 else b.act_scale for b in blocks])
    record = ref.zero_record(N); nxt = []
    for s, (q, se, obs, rew, gl, rst) in enumerate(stream):
        nxt.append(ref.update(plan, record, s, q, se, obs, rew, gl, rst))
    return plan, record, nxt


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.int32), np.ascontiguousarray(b, dtype=np.float32).view(np.int32))


# ---------------------------------------------------------------------------------------------------------------- torch path == reference
@pytest.mark.parametrize("cmd_mode", [ref.CMD_ACTIONS, ref.CMD_TARGETS])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_torch_path_equals_reference_bit_for_bit(robot_model, family, cmd_mode):
    params, split = FAMILIES[family]()
    N = 32
    recs, cmds, env_rec, stream = synthetic_case(params, split, N, cmd_mode)
    eng = OracleEngine(robot_model, params, N, split, 0, 5.0, 1.0)
    kw = dict(actions=cmds) if cmd_mode == ref.CMD_ACTIONS else dict(targets=cmds)
    plan = ReplayPlan(eng, recs, env_rec, hold=HOLD, window_rows=WINDOW, track_tol=TOL, **kw)
    assert plan.pd and plan.cmd_mode == cmd_mode and plan.steps == max(LENS) + HOLD and plan.v2_thresh == V2_THRESH
    rplan, want, want_next = reference_run(params, split, recs, cmds, env_rec, stream, cmd_mode)
    assert rplan.steps() == plan.steps and same_bits(plan.inv_scale_t.numpy(), rplan.inv_scale)
    record = ReplayRecord(eng); record.record[:, env_rec < 0] = 777.0
    actions = torch.full((N, 12), 9.0)
    for s, (q, se, obs, rew, gl, rst) in enumerate(stream):
        eng.state[13:25] = torch.from_numpy(q); eng.state[90:102] = torch.from_numpy(se)
        eng.cnt[2] = torch.from_numpy(gl); eng.cnt[3] = torch.from_numpy(rst)
        record.update(plan, s, torch.from_numpy(obs), torch.from_numpy(rew), actions)
        assert same_bits(actions.numpy(), want_next[s]), s
    got = record.record.numpy(); part = env_rec >= 0
    assert (got[:, ~part] == 777.0).all()
    for r in range(ref.ROWS):
        assert same_bits(got[r, part], want[r, part]), (r, got[r, part], want[r, part])
    assert (got[30:, part] == 0).all()
    # the cases the stream was built to hold
    assert want[ref.FINISHED, 0] == 1 and want[ref.DONE_AT, 0] == 0 and want[ref.ROWS_, 0] == 1
    assert want[ref.FINISHED, 2] == 0 and want[ref.ROWS_, 2] == LENS[2] and want[ref.FINISHED, 3] == 0 and want[ref.ROWS_, 3] == LENS[0]
    assert (want_next[LENS[0] - 1][3] == 0).all() and (want_next[LENS[0] - 2][3] != 0).any()          # s + 1 == T: no further action
    assert (want[ref.FINISHED, part] == 1).sum() >= 8
    if cmd_mode == ref.CMD_TARGETS:
        sat = want[ref.SATURATED, part]
        assert sat.max() > 12 and (np.abs(np.stack(want_next)) < 1.0).any() and (np.abs(np.stack(want_next)) == 1.0).any()
        if family == "pos":
            assert (want[ref.CMD_ERR] == 0).all()
        else:
            assert want[ref.CMD_ERR, 2] > 1.0          # targets far outside [se_lo, se_hi] cannot be held
    else:
        assert (want[ref.SATURATED] == 0).all() and (want[ref.CMD_ERR] == 0).all()
    s = record.summary()
    assert np.array_equal(s["saturated"][part], want[ref.SATURATED, part].astype(np.int64)) and same_bits(s["cmd_err"][part], want[ref.CMD_ERR, part])


def test_se_command_inverts_the_steps_target_map():
    rng = np.random.default_rng(0)
    p = loco_cc_params()
    se = rng.uniform(p.se_lo, p.se_hi, (200, 12)).astype(np.float32)
    err = max(np.abs(ref.se_command(ref.joint_targets(x)).astype(np.float64) - x).max() for x in se)
    print("largest round-trip error of the target map: %.3e (bound %.3e)" % (err, MAP_ROUNDING))
    assert err <= MAP_ROUNDING


# ---------------------------------------------------------------------------------------------------------------- keyword rules, refusals
def test_keyword_rules_and_refusals(robot_model):
    rng = np.random.default_rng(1)
    rec = np.cumsum(rng.uniform(-0.05, 0.05, (20, 12)), axis=0); act = rng.uniform(-1, 1, (20, 12))
    ids = np.full(16, -1, dtype=np.int32); ids[3] = 0
    vel = OracleEngine(robot_model, [loco_params()], 16, None, 0, 5.0, 1.0)
    with pytest.raises(ValueError, match="targets"):
        ReplayPlan(vel, [rec], ids, targets=[rec], window_rows=4)
    assert not ReplayPlan(vel, [rec], ids, window_rows=4).pd and not ReplayPlan(vel, [rec], ids, actions=[act], servo=True, window_rows=4).pd
    eff = OracleEngine(robot_model, [loco_params(drive_mode=2)], 16, None, 0, 5.0, 1.0)
    with pytest.raises(ValueError, match="targets"):
        ReplayPlan(eff, [rec], ids, targets=[rec], window_rows=4)
    with pytest.raises(ValueError, match="variant 0 in velocity drive"):
        ReplayPlan(eff, [rec], ids, actions=[act], window_rows=4)
    for make in (loco_cc_params, loco_pc_params, lambda: loco_params(drive_mode=1, act_scale=3.14159)):
        pd = OracleEngine(robot_model, [make()], 16, None, 0, 5.0, 1.0)
        with pytest.raises(ValueError, match="variant 0 in velocity drive"):          # no command log: refused as before
            ReplayPlan(pd, [rec], ids, window_rows=4)
        a = ReplayPlan(pd, [rec], ids, actions=[act], window_rows=4)
        t = ReplayPlan(pd, [rec], ids, targets=[rec + 0.01], window_rows=4)
        v = ReplayPlan(pd, [rec], ids, servo=True, window_rows=4)
        assert (a.pd, a.cmd_mode, t.cmd_mode, v.cmd_mode) == (True, ref.CMD_ACTIONS, ref.CMD_TARGETS, ref.CMD_TARGETS) and a.steps == 22
        assert np.array_equal(v.act_t.numpy(), v.rec_t.numpy()) and np.array_equal(a.act_t[0].numpy(), act.astype(np.float32))          # servo: the recordings are the targets
        assert a.full is None
        nan_t = rec.copy(); nan_t[7, 2] = np.nan
        for bad in (dict(actions=[act], targets=[rec]), dict(actions=[act], servo=True), dict(targets=[rec], servo=True), dict(targets=[rec[:-1]]),
                    dict(actions=[act, act]), dict(targets=[nan_t]), dict(actions=[np.where(np.arange(20)[:, None] == 3, np.inf, act)]), dict(servo=True, hold=9),
                    dict(servo=True, window_rows=21), dict(servo=True, env_rec=np.where(ids >= 0, 1, -1).astype(np.int32)), dict(servo=True, env_rec=ids[:15])):
            with pytest.raises(ValueError):
                ReplayPlan(**{**dict(engine=pd, recordings=[rec], env_rec=ids, window_rows=4), **bad})
    mixed = OracleEngine(robot_model, [loco_pc_params(), loco_params()], 32, 16, 0, 5.0, 1.0)          # one PD block is not enough
    with pytest.raises(ValueError, match="targets"):
        ReplayPlan(mixed, [rec], np.full(32, -1, dtype=np.int32), targets=[rec], window_rows=4)


def test_abi_of_the_pd_entry_point():
    lmlib.build_library()
    so = lmlib.load_library()
    assert "lm_replay_create_pd" in lmlib.EXPORTS and hasattr(so, "lm_replay_create_pd")
    assert (lmlib.REPLAY_CMD_ACTIONS, lmlib.REPLAY_CMD_TARGETS, lmlib.REPLAY_SATURATED, lmlib.REPLAY_CMD_ERR) == (0, 1, ref.SATURATED, ref.CMD_ERR)
    h = C.c_void_p(); one = (C.c_float * 12)(); ids = (C.c_int32 * 1)(0)
    assert so.lm_replay_create_pd(None, None, None, None, None, 1, 1, None, 0, 0, 1, 1.0, 1.0) == -1 and b"null" in so.lm_last_error()
    assert so.lm_replay_create_pd(C.byref(h), None, one, one, ids, 1, 1, ids, 0, 0, 1, 1.0, 1.0) == -1 and b"null" in so.lm_last_error() and not h


# ---------------------------------------------------------------------------------------------------------------- oracle walk: record, replay
# The target map and its inverse in fp32, |se| < 2.35 so |targets| < 4 and |dof2 + dof3| < 8.  Forward: dof2 = fl(swing + ext / 2) and
# dof3 = fl(swing - ext / 2) are each off by at most half an ulp of [2, 4), 2^-23 (ext / 2 is exact).  Inverse: swing' = fl(dof2 + dof3) / 2 carries
# (2^-23 + 2^-23) / 2 from the forward errors plus half an ulp of [4, 8) halved, 2^-23: at most 2^-22.  ext' = fl(dof2 - dof3) carries
# 2^-23 + 2^-23 plus half an ulp of [2, 4): at most 3 x 2^-23.  That is the distance between the logged command and the command a replay is
# asked to hold.  The replayed engine then holds the asked command to 1.2 x 2^-23 (its own fl(se + fl(a x scale)) with a = fl(fl(c - se) x inv):
# half an ulp of the sum, 2^-23, plus three relative roundings of 2^-24 on a step of at most 0.1), or, where the asked command lies outside
# [se_lo, se_hi] by its rounding, the limit itself: at most the map's 3 x 2^-23 away.  So cmd_err <= 3 x 2^-23 = 3.58e-7.
MAP_ROUNDING = 3.0 * 2.0 ** -23
WALK_ROWS, WALK_N, SRC_ENVS, DST_ENVS = 24, 16, (2, 11), (5, 14)


def walk(robot_model, make, seed=3):
    """A source engine under seeded random actions (row 0: the reset step, zero actions): per tracked env the joints, the applied actions and
    the joint position targets read back from the R_SE rows, one row per step."""
    eng = OracleEngine(robot_model, [make()], WALK_N, None, 0, 5.0, 1.0, precision="f32")
    rng = np.random.default_rng(seed)
    obs = torch.empty(WALK_N, eng.num_obs); rew = torch.empty(WALK_N)
    rows = {e: dict(q=[], actions=[], targets=[]) for e in SRC_ENVS}
    for t in range(WALK_ROWS):
        act = np.zeros((WALK_N, 12), dtype=np.float32) if t == 0 else rng.uniform(-0.9, 0.9, (WALK_N, 12)).astype(np.float32)
        eng.step(torch.from_numpy(act), out_obs=obs, out_rew=rew)
        for e in SRC_ENVS:
            assert t == WALK_ROWS - 1 or int(eng.cnt[3, e]) == 0, (e, t)          # the walk does not end before its last row
            rows[e]["q"].append(eng.state[13:25, e].numpy().copy()); rows[e]["actions"].append(act[e].copy())
            rows[e]["targets"].append(ref.joint_targets(eng.state[90:102, e].numpy()))
    return [{k: np.stack(v) for k, v in rows[e].items()} for e in SRC_ENVS]


@pytest.mark.parametrize("make", [loco_cc_params, loco_pc_params], ids=["cc", "pc"])
def test_oracle_walk_replays_from_its_action_log_and_from_its_target_log(robot_model, make):
    logs = walk(robot_model, make)
    env_rec = np.full(WALK_N, -1, dtype=np.int32); env_rec[list(DST_ENVS)] = [0, 1]
    out = {}
    for mode, kw in (("actions", dict(actions=[g["actions"] for g in logs])), ("targets", dict(targets=[g["targets"] for g in logs]))):
        eng = OracleEngine(robot_model, [make()], WALK_N, None, 0, 5.0, 1.0, precision="f32")
        plan = ReplayPlan(eng, [g["q"] for g in logs], env_rec, hold=0, window_rows=4, **kw)
        out[mode] = plan.run(ReplayRecord(eng)).summary()
        print(mode, {k: out[mode][k][list(DST_ENVS)] for k in ("rows", "qerr", "rms", "saturated", "cmd_err")})
    for e in DST_ENVS:
        assert out["actions"]["qerr"][e] == 0.0 and out["actions"]["rows"][e] == WALK_ROWS and out["actions"]["row0_err"][e] == 0.0
        assert out["actions"]["saturated"][e] == 0 and out["actions"]["cmd_err"][e] == 0.0          # neither row is written in actions mode
        assert out["targets"]["rows"][e] == WALK_ROWS and out["targets"]["saturated"][e] == 0
        assert out["targets"]["cmd_err"][e] <= MAP_ROUNDING, (e, out["targets"]["cmd_err"][e])
        assert out["targets"]["qerr"][e] < 1e-3          # and the joints follow (not exact: the recovered actions carry the map's rounding)
