"""Replay of recorded joint motions on the GPU (include/lm_policy.h, csrc/lm_replay.hip).

1. k_replay_update alone on synthetic state written into the engine's zero-copy views, against the float64 reference
   (tests/replay_reference.py): exact integer rows (every threshold comparison kept >= 1e-4 from its threshold by construction, asserted on
   the CPU), float rows to 1e-5 relative, the action table copied / the servo expression bit for bit, guards, idle envs, frozen finished envs.
2. The device replay of the 11 recordings at two friction coefficients on one co-training engine against npy_replay.replay() looped from the
   host through Engine.step on an identical second engine.
3. Record -> replay round trip: what TrajectoryRecord wrote replays to qerr == 0.0 exactly on another engine at other env indices; with mu
   halved it does not.
4. The friction grid of tests/test_reference_npy_replay.py plus two far points in ONE run; 5. the servo replays; 6. the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import npy_replay as R
import replay_reference as ref
import test_reference_npy_replay as T

pytestmark = pytest.mark.gpu

GUARD = 0x7FC0BEEF          # an int32 bit pattern (a NaN payload) nothing writes
V2_THRESH = float(np.float32(np.sin(0.075) ** 2))


@pytest.fixture(scope="module")
def recordings():
    return R.load()


@pytest.fixture(scope="module")
def lmlib():
    from locomanipulationrl_amd import lib
    lib.build_library()
    return lib


def cotrain_blocks():
    return [R.cotrain_params("loco"), R.cotrain_params("mani")]


KINDS = {n: R.kind_of(n) for n in R.FILES}


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel alone
N1, LENS1, WINDOW1, HOLD1, TOL1 = 40, (5, 19, 23), 4, 2, 1e-3


def synthetic_case(seed=7):
    """Three recordings, the env map (idle envs in the first and in the last, partial, group), and per step what lm_step would have left:
    q (12, N), obs (N, 64), rewards (N,), goal and reset flags (N,).  Joint-step errors are drawn from [0, 8e-4] or [1.2e-3, 5e-3] and |v|^2
    from [0, 5.0e-3] or [6.2e-3, 0.5], so no comparison comes near track_tol = 1e-3 or v2_thresh = 5.61e-3."""
    rng = np.random.default_rng(seed)
    recs = [np.cumsum(rng.uniform(-0.08, 0.08, (L, 12)), axis=0) + rng.uniform(-1.0, 1.0, 12) for L in LENS1]
    env_rec = rng.integers(0, 3, N1).astype(np.int32)
    env_rec[[0, 1, 2, 3, 4, 5]] = [0, 1, 2, 0, 1, 2]
    env_rec[[6, 17, 33, 39]] = -1
    steps = max(LENS1) + HOLD1 + 2          # two calls past the last scored row: nothing may change any more
    T_of = np.array([LENS1[r] if r >= 0 else 0 for r in env_rec])
    # when each env raises its reset flag (-1: never): on row 0, inside the recording, on its last row, on a hold row, never
    done_at = np.where(rng.random(N1) < 0.6, rng.integers(1, np.maximum(T_of, 2)), -1)
    done_at[[0, 1, 2, 3, 4, 5]] = [0, 18, -1, 4, 19, 24]          # row 0 | last row | never | last row | first hold row | second hold row
    goal = rng.random(N1) < 0.5
    stream = []
    noise = rng.uniform(-2e-3, 2e-3, (12, N1))
    for s in range(steps):
        if s >= 1:
            mag = np.where(rng.random((12, N1)) < 0.7, rng.uniform(0.0, 8e-4, (12, N1)), rng.uniform(1.2e-3, 5e-3, (12, N1)))
            noise = noise + mag * rng.choice([-1.0, 1.0], (12, N1))
        q = np.stack([recs[max(r, 0)][min(s, T_of[e] - 1 if r >= 0 else 0)] for e, r in enumerate(env_rec)], axis=1) + noise
        obs = rng.uniform(-5.0, 5.0, (N1, 64))
        inside = rng.random(N1) < min(1.0, s / 12.0)          # the orientation error shrinks along the replay
        v2 = np.where(inside, rng.uniform(0.0, 5.0e-3, N1), rng.uniform(6.2e-3, 0.5, N1))
        d = rng.normal(size=(N1, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        obs[:, 7:10] = d * np.sqrt(v2)[:, None]
        rew = rng.uniform(0.5, 3.0, N1)
        # after its first reset flag an env keeps raising flags at random: a finished env must stay frozen whatever it sees
        rst = (done_at == s) | ((done_at >= 0) & (s > done_at) & (rng.random(N1) < 0.3))
        stream.append((q.astype(np.float32), obs.astype(np.float32), rew.astype(np.float32), (goal ^ (rng.random(N1) < 0.2)).astype(np.int64), rst.astype(np.int64)))
    return recs, env_rec, stream


def reference_run(recs, acts, env_rec, stream, servo, inv_full):
    Tm = max(LENS1)
    rec = np.zeros((3, Tm, 12), dtype=np.float32); act = np.zeros_like(rec)
    for k in range(3):
        rec[k, :LENS1[k]] = recs[k]; act[k, :LENS1[k]] = acts[k]
    plan = ref.Plan(rec, act, LENS1, env_rec, servo, HOLD1, WINDOW1, inv_full, V2_THRESH, float(np.float32(TOL1)))
    record = ref.zero_record(N1); nxt, go, margin = [], [], [np.inf, np.inf]
    for s, (q, obs, rew, gl, rst) in enumerate(stream):
        a, b = ref.margins(plan, record, s, q, obs); margin = [min(margin[0], a), min(margin[1], b)]
        nxt.append(ref.update(plan, record, s, q, obs, rew, gl, rst))
        go.append(np.array([r >= 0 and record[ref.FINISHED, e] == 0 and s + 1 < LENS1[r] for e, r in enumerate(env_rec)]))
    return plan, record, nxt, go, margin


@pytest.mark.parametrize("servo", [False, True])
def test_kernel_on_synthetic_state(robot_model, lmlib, servo):
    from locomanipulationrl_amd.engine_config import loco_params
    recs, env_rec, stream = synthetic_case()
    rng = np.random.default_rng(11)
    acts = [rng.uniform(-1.0, 1.0, a.shape) for a in recs]
    eng = lmlib.Engine(robot_model, [loco_params()], N1, seed=3)
    plan = lmlib.ReplayPlan(eng, recs, env_rec, actions=acts, servo=servo, hold=HOLD1, window_rows=WINDOW1, track_tol=TOL1)
    assert plan.steps == max(LENS1) + HOLD1 and plan.v2_thresh == V2_THRESH
    rplan, want, want_next, go, margin = reference_run(recs, acts, env_rec, stream, servo, plan.inv_full)
    print("threshold margins: track_tol %.3e, v2_thresh %.3e" % tuple(margin))
    assert margin[0] >= 1e-4 and margin[1] >= 1e-4
    part = env_rec >= 0; idle = torch.from_numpy(~part).cuda()
    assert 3 <= (~part).sum() and (want[ref.FINISHED, part] == 1).sum() >= 10 and (want[ref.FINISHED, part] == 0).sum() >= 3

    def run():
        whole = torch.empty((lmlib.REPLAY_ROWS + 2, N1), dtype=torch.float32, device="cuda"); whole.view(torch.int32).fill_(GUARD)
        rec = lmlib.ReplayRecord(eng); rec.record = whole[1:-1]; rec.zero()
        rec.record[:, idle] = 777.0                                         # the columns of the idle envs must come back as they are
        awhole = torch.empty((N1 + 2, 12), dtype=torch.float32, device="cuda"); awhole.view(torch.int32).fill_(GUARD)
        actions = awhole[1:-1]
        assert rec.record.is_contiguous() and actions.is_contiguous() and actions.data_ptr() % 16 == 0
        seen, frozen = [], None
        for s, (q, obs, rew, gl, rst) in enumerate(stream):
            eng.state[13:25] = torch.from_numpy(q).cuda(); eng.cnt[2] = torch.from_numpy(gl).cuda(); eng.cnt[3] = torch.from_numpy(rst).cuda()
            actions.fill_(9.0)
            rec.update(plan, s, torch.from_numpy(obs).cuda(), torch.from_numpy(rew).cuda(), actions)
            seen.append(actions.clone())
            if s == plan.steps - 1:
                frozen = rec.record.clone()
        torch.cuda.synchronize()
        assert (whole[0].view(torch.int32) == GUARD).all() and (whole[-1].view(torch.int32) == GUARD).all()
        assert (awhole[0].view(torch.int32) == GUARD).all() and (awhole[-1].view(torch.int32) == GUARD).all()
        assert torch.equal(frozen, rec.record)                              # the two calls past the last row changed nothing
        return rec.record.clone(), torch.stack(seen)

    got, seen = run()
    g = got.double().cpu().numpy()
    assert (g[:, ~part] == 777.0).all() and (g[28:, part] == 0.0).all()
    for r in ref.INTEGER_ROWS:
        assert np.array_equal(g[r, part], want[r, part]), (r, g[r, part], want[r, part])
    for r in ref.FLOAT_ROWS:
        assert (np.abs(g[r, part] - want[r, part]) <= 1e-5 * np.abs(want[r, part])).all(), (r, g[r, part], want[r, part])
    # actions_next: zero for idle, finished and exhausted envs; otherwise the table's row (a copy) or the servo expression in fp32, bit for bit
    rec_t, act_t, ids = plan.rec_t.cpu(), plan.act_t.cpu(), torch.from_numpy(np.maximum(env_rec, 0)).long()
    for s, (q, *_rest) in enumerate(stream):
        k = min(s + 1, plan.T_max - 1)
        full_row = ((rec_t[ids, k] - torch.from_numpy(q).T) * plan.inv_full).clamp(-1.0, 1.0) if servo else act_t[ids, k]
        expect = torch.where(torch.from_numpy(go[s])[:, None], full_row, torch.zeros(N1, 12))
        assert torch.equal(seen[s].cpu(), expect), s
        assert np.abs(expect.double().numpy() - want_next[s]).max() <= 2e-6          # (and that is what the reference asks for)
    assert any(g_.any() for g_ in go)
    # a finished env stays frozen: its column after the step that finished it is its column at the end (seen through the reference, which
    # matched above, and directly for env 0, finished on row 0)
    assert g[ref.FINISHED, 0] == 1 and g[ref.DONE_AT, 0] == 0 and g[ref.ROWS_, 0] == 1
    got2, seen2 = run()
    assert torch.equal(got.view(torch.int32), got2.view(torch.int32)) and torch.equal(seen.view(torch.int32), seen2.view(torch.int32))
    plan.close(); eng.close()


# ---------------------------------------------------------------------------------------------------------------- 2. device replay == host-looped twin
def test_device_replay_equals_the_host_looped_replay(robot_model, lmlib, recordings):
    """7 locomotion files x 2 points padded to 16 and 4 manipulation files x 2 points padded to 16, mu held at 0.8 and 0.4, against
    npy_replay.replay(until_done=True) through Engine.step on an identical second engine, reading the same env.  The integer outcomes are
    exact.  Joint errors and min_rd agree to 1e-5 absolute (the twin subtracts the fp64 recording, the device its fp32 copy: 6e-8 rad), the
    returns to 1e-5 relative (fp32 sums of ~100 positive terms against fp64 sums of the same fp32 terms)."""
    from locomanipulationrl_amd.train import replay as RP
    points = [{"mu": 0.8}, {"mu": 0.4}]
    recs = {n: recordings[n] for n in R.FILES}
    out = RP.replay_sweep(robot_model, cotrain_blocks(), recs, KINDS, points, hold=2)
    lay = out["layout"]
    assert (lay["num_envs"], lay["split"]) == (32, 16) and out["steps"] == max(len(a) for a in recs.values()) + 2
    twin = RP.sweep_engine(robot_model, cotrain_blocks(), lay, points)
    twin.obs_buf                                         # the unclipped observations are read below: ask for them before the first step
    N = lay["num_envs"]
    o_obs = torch.empty(N, 64, device="cuda"); o_rew = torch.empty(N, device="cuda")
    for p in range(2):
        for name in R.FILES:
            e = lay["env_of"][(name, p)]
            twin.reset_all()

            def step(a, e=e):
                act = torch.as_tensor(np.asarray(a, dtype=np.float32), device="cuda").repeat(N, 1).contiguous()
                twin.step(act, out_obs=o_obs, out_rew=o_rew)
                torch.cuda.synchronize()
                return (twin.state[13:25, e].double().cpu().numpy(), twin.obs_buf[e].double().cpu().numpy(), int(twin.cnt[3, e]), int(twin.cnt[2, e]), float(o_rew[e]))
            want = R.replay(recs[name], step, until_done=True)
            got = out["runs"][p][name]
            print(name, points[p], "device:", {k: got[k] for k in ("rows", "done_at", "goal", "first_succ", "in_window")}, "qerr %.4f min_rd %.4f ret %.2f" % (got["qerr"], got["rd_rec"][0], got["ret"]))
            L = len(recs[name])
            assert got["rows"] == len(want["rows"]) and got["done_at"] == want["done_at"] and got["goal"] == want["goal"], (name, p, got, want["done_at"], want["goal"])
            assert got["first_succ"] == want["first_succ"] and got["in_window"] == want["in_window"], (name, p, got["first_succ"], want["first_succ"])
            assert abs(got["row0_err"] - want["row0_err"]) <= 1e-5 and abs(got["qerr"] - want["qerr"]) <= 1e-5, (name, p)
            assert abs(got["rd_rec"][0] - want["rd_rec"].min()) <= 1e-5 and abs(got["rd"][0] - want["rd"][0]) <= 1e-5, (name, p)
            for a, b in ((got["ret"], want["rew"].sum()), (got["window_return"], want["rew"][L - 17:L].sum())):
                assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (name, p, a, b)
    twin.close()
    # the two columns differ: friction decides behaviour
    assert any(out["runs"][0][n]["in_window"] != out["runs"][1][n]["in_window"] for n in R.GOAL_KNOWN)


# ---------------------------------------------------------------------------------------------------------------- 3. record -> replay round trip
def test_record_replay_round_trip(robot_model, lmlib):
    """TrajectoryRecord (episode cap 1) under random actions on a locomotion engine with max_episode 12, envs 5 and 37; the recorded q and
    last_actions replayed on a second engine at envs 9 and 50 give the recording back exactly (qerr == 0.0: the engine is deterministic and an
    env's trajectory does not depend on its index), and at envs 10 and 51, where mu is held at half the nominal value, they do not.
    The joints are velocity-driven, so friction moves them little: over the envs of such a walk the CPU oracle's median deviation under half
    friction is 1.0e-3 rad, the bound itself.  The action seed (18, host generator) is the first of 0 .. 149 for which the oracle - fp32 and
    fp64 alike - predicts twice the bound for both tracked envs (2.08e-3 and 2.04e-3 rad, both episodes 11 rows)."""
    from locomanipulationrl_amd.engine_config import loco_params
    N, ids = 64, [5, 37]
    ep = loco_params(max_episode=12, dr_enabled=1)
    a = lmlib.Engine(robot_model, [ep], N, seed=1); a.enable_env_params(); a.set_env_params(mu=ep.mu)
    traj = lmlib.TrajectoryRecord(a, ids, 16, episode_cap=1)
    g = torch.Generator().manual_seed(18)
    rew = torch.empty(N, device="cuda"); rst = torch.empty(N, dtype=torch.int64, device="cuda")
    for t in range(14):
        act = torch.zeros(N, 12, device="cuda") if t == 0 else (torch.rand(N, 12, generator=g) * 2.0 - 1.0).cuda()
        a.step(act, out_rew=rew, out_resets=rst); traj.update(rew, rst)
    eps = [traj.episodes(k)[0] for k in range(2)]
    a.close()
    assert all(e["complete"] and not e["truncated"] and 4 <= len(e["q"]) <= 12 for e in eps), [len(e["q"]) for e in eps]
    b = lmlib.Engine(robot_model, [ep], N, seed=1); b.enable_env_params()
    mu = np.full(N, ep.mu, dtype=np.float32); mu[[10, 51]] = 0.5 * ep.mu
    b.set_env_params(mu=mu)
    env_rec = np.full(N, -1, dtype=np.int32); env_rec[[9, 50, 10, 51]] = [0, 1, 0, 1]
    plan = lmlib.ReplayPlan(b, [e["q"] for e in eps], env_rec, actions=[e["last_actions"] for e in eps], hold=0, window_rows=4)
    s = plan.run(lmlib.ReplayRecord(b)).summary()
    print({k: v[[9, 50, 10, 51]] for k, v in s.items()})
    for env, e in ((9, eps[0]), (50, eps[1])):
        assert s["qerr"][env] == 0.0 and s["row0_err"][env] == 0.0 and s["done_at"][env] == len(e["q"]) - 1 and s["tracked"][env] == 1.0 and s["rows"][env] == len(e["q"])
        # (the returns are not compared: the goal of an episode is drawn per env index, and the reward follows the goal; the joints do not)
    for env in (10, 51):
        assert s["qerr"][env] > 1e-3, (env, s["qerr"][env])          # the negative control
    plan.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------- 4. the friction grid in one run
def test_friction_grid_in_one_run(robot_model, lmlib, recordings):
    """MU_GRID of tests/test_reference_npy_replay.py plus 0.0 and 1.6: 13 points x (7 + 4) files = 91 -> 96 and 52 -> 64 envs.  The shipped
    column (0.8) passes the drive-limit and orientation checks of that file; the two far columns fail the orientation checks.  The
    leave-one-out picks are printed, not asserted (fp32 chaos can move a tie)."""
    from locomanipulationrl_amd.train import replay as RP
    grid = sorted(set(T.MU_GRID) | {0.0, 1.6})
    points = [{"mu": m} for m in grid]
    out = RP.replay_sweep(robot_model, cotrain_blocks(), {n: recordings[n] for n in R.FILES}, KINDS, points, hold=2, score_files=R.GOAL_KNOWN)
    assert len(grid) == 13 and (out["layout"]["split"], out["layout"]["num_envs"]) == (96, 160)
    for p, m in enumerate(grid):
        print("mu %.2f rows in PhysX's window per file %s shared %d" % (m, out["in_window"][p], out["shared"][p]))
    print("leave-one-out:", [(n, grid[p], rows) for n, p, rows in out["leave_one_out"]])
    shipped = out["runs"][grid.index(0.8)]
    for name, r in shipped.items():
        print(R.summary_line(name, {**r, "rd_rec": np.array([r["rd_rec"][0], r["rd_rec"][0]])}))
    T.check_drive_limit(shipped)
    T.check_orientation(shipped)
    assert not T.orientation_ok(out["runs"][grid.index(0.0)]) and not T.orientation_ok(out["runs"][grid.index(1.6)])


# ---------------------------------------------------------------------------------------------------------------- 5. servo
def test_servo_replays_stay_on_the_recording(robot_model, lmlib, recordings):
    """All 11 files at the shipped point, steered back onto the recording every step: the thresholds of
    test_servo_replay_keeps_the_joints_on_the_recording."""
    from locomanipulationrl_amd.train import replay as RP
    out = RP.replay_sweep(robot_model, cotrain_blocks(), {n: recordings[n] for n in R.FILES}, KINDS, [{"mu": 0.8}], servo=True, hold=0)
    for name, r in out["runs"][0].items():
        print(name, "qerr %.4f mean |error| %.5f rows %d" % (r["qerr"], r["mean_abs"], r["rows"]))
        assert r["qerr"] <= 0.05 and r["mean_abs"] < 2e-3, (name, r["qerr"], r["mean_abs"])


# ---------------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_through_ctypes(robot_model, lmlib, recordings):
    from locomanipulationrl_amd.engine_config import loco_cc_params, loco_params, loco_pc_params
    N = 16
    rec = np.ascontiguousarray(recordings["test"], dtype=np.float32); L = len(rec)
    act = np.zeros_like(rec); lens = np.array([L], dtype=np.int32); ids = np.zeros(N, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def create(eng, rec=rec, lens=lens, ids=ids, hold=2, window=17, T_max=L, scal=(10.0, 0.0056, 1e-3)):
        h = C.c_void_p()
        rc = eng.lib.lm_replay_create(C.byref(h), eng._h, p(rec), p(act), p(lens), 1, T_max, p(ids), 0, hold, window, *scal)
        return rc, h, eng.lib.lm_last_error()

    for make, word in ((loco_cc_params, b"variant 0"), (loco_pc_params, b"variant 0"), (lambda: loco_params(drive_mode=1, act_scale=3.14159), b"velocity drive")):
        eng = lmlib.Engine(robot_model, [make()], N, seed=1)
        rc, h, msg = create(eng)
        assert rc == -1 and not h and word in msg, (rc, msg)
        with pytest.raises(lmlib.EngineError):
            lmlib.ReplayPlan(eng, [recordings["test"]], ids)
        eng.close()
    eng = lmlib.Engine(robot_model, [loco_params()], N, seed=1)
    state0, cnt0 = eng.state.clone(), eng.cnt.clone()
    bad_id, low_id = ids.copy(), ids.copy(); bad_id[7] = 1; low_id[3] = -2
    nan_rec = rec.copy(); nan_rec[5, 3] = np.nan
    for kw, word in ((dict(ids=bad_id), b"recording id"), (dict(ids=low_id), b"recording id"), (dict(lens=np.array([L + 1], dtype=np.int32)), b"length"),
                     (dict(lens=np.array([16], dtype=np.int32)), b"length"), (dict(hold=9), b"hold"), (dict(hold=-1), b"hold"), (dict(rec=nan_rec), b"finite"),
                     (dict(scal=(float("inf"), 0.0056, 1e-3)), b"finite"), (dict(T_max=0), b"T_max")):
        rc, h, msg = create(eng, **kw)
        assert rc == -1 and not h and word in msg, (kw.keys(), rc, msg)
    rc, h, msg = create(eng)
    assert rc == 0 and h and eng.lib.lm_replay_steps(h) == L + 2
    obs = torch.zeros(N, 64, device="cuda"); rew = torch.zeros(N, device="cuda"); record = torch.zeros(32, N, device="cuda"); nxt = torch.full((N, 12), 3.0, device="cuda")
    P = lmlib.Engine._p
    assert eng.lib.lm_replay_update(h, -1, P(obs), P(rew), P(record), P(nxt), None) == -1 and b"negative" in eng.lib.lm_last_error()
    assert eng.lib.lm_replay_update(h, 0, P(obs), None, P(record), P(nxt), None) == -1 and b"null" in eng.lib.lm_last_error()
    assert eng.lib.lm_replay_update(h, 0, P(obs), P(rew), P(record), C.c_void_p(nxt.data_ptr() + 4), None) == -1 and b"aligned" in eng.lib.lm_last_error()
    torch.cuda.synchronize()
    assert (record == 0).all() and (nxt == 3.0).all() and torch.equal(eng.state, state0) and torch.equal(eng.cnt, cnt0)          # nothing was written
    assert eng.lib.lm_replay_destroy(h) == 0
    eng.close()
