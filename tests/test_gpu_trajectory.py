"""The trajectory record on the GPU (include/lm_policy.h): k_trajectory_update behind the enqueue and graph rollouts and behind
lm_trajectory_update against the independent numpy reference (tests/trajectory_reference.py).  Every comparison of rows and headers is
exact (bit patterns): the record is a copy.  The persistent kernel keeps the record on the MLP with 64-wide observations (k_rollout_mlp_tr,
every combination with deterministic mode and an episode record); where no such build ships - 88-wide observations, randomised engines,
contact reporting - "persistent" is asserted to be refused and the third plan runs "auto", which takes the graph.  Columns 43-54 (R_LTIP)
are documented as base-frame tips, not world positions, so there is no comparison with lm_forward_kinematics.

Episodes are shortened through the parameter block (max_episode = 6: an episode every 5 steps), T = 7 and every engine is about to reset
when the record starts, so the first episode ends inside the first run (step 5) and the second one begins in the first run and ends in the
second (step 10)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import trajectory_reference as tr

pytestmark = pytest.mark.gpu

T = 7
MODES = ("enqueue", "graph", "persistent")
BUFFERS = ("obs", "actions", "logp", "values", "rewards", "dones", "extras")
GUARD = 0x7FC0BEEF          # an int32 bit pattern (a NaN payload) no row holds


def make_task(task_name, N):
    from locomanipulationrl_amd.utils.config import SimConfig, load_config
    from locomanipulationrl_amd.utils.task_util import task_map
    return task_map()[task_name](name=task_name, sim_config=SimConfig(load_config(task_name, num_envs=N)), env=None)


def make_policy(task):
    from locomanipulationrl_amd.lib import POLICY_MLP
    from locomanipulationrl_amd.policies.mlp_model import SharedMLP, pack_mlp_params
    model = SharedMLP(num_observations=task.engine_params()[0].num_obs).cuda()
    return POLICY_MLP, pack_mlp_params(model, None, None).cuda()


def make_engine(task, N, params, seed=9):
    from locomanipulationrl_amd.lib import Engine
    from locomanipulationrl_amd.model.robot_model import load_model
    return Engine(load_model(task.model_asset), params, N, split_env=task.split_env(), seed=seed)


def first_obs(e):
    o0 = torch.empty(e.num_envs, e.num_obs, device="cuda"); e.step(torch.zeros(e.num_envs, 12, device="cuda"), None, o0)
    return o0


def make_plan(e, kind, packed, log_std, **switches):
    from locomanipulationrl_amd.lib import Rollout
    r = Rollout(e, kind, packed, log_std, T, noise_seed=21, **switches)
    r.obs[0] = first_obs(e)
    return r


def same_engines(a, b):
    return torch.equal(a.state, b.state) and torch.equal(a.cnt, b.cnt) and torch.equal(a.stats_i64, b.stats_i64)


def guarded_record(e, ids, max_rows, cap):
    """A TrajectoryRecord whose rows are followed, in the same allocation, by one guard slot filled with a bit pattern."""
    from locomanipulationrl_amd.lib import TrajectoryRecord
    rec = TrajectoryRecord(e, ids, max_rows, episode_cap=cap)
    whole = torch.empty((len(ids) + 1, max_rows, 64), dtype=torch.float32, device="cuda")
    whole.view(torch.int32).fill_(GUARD)
    rec.rows = whole[:len(ids)]; rec.rows.zero_()
    rec.guard = whole[len(ids):]
    assert rec.rows.data_ptr() % 16 == 0 and rec.rows.is_contiguous()
    return rec


def guard_intact(rec):
    return bool((rec.guard.view(torch.int32) == GUARD).all())


def drive(task_name, N, ids, max_rows=2 * T, cap=0, det=False, episode=False, changes=None, setup=None, runs=2, seed=31, persistent=True):
    """Twin engines, one plan per mode, and a further twin stepped by hand (Engine.step on the first plan's actions +
    TrajectoryRecord.update) that also feeds the numpy reference.  After every run all records must hold the reference's bits.
    persistent=False: the plan's persistent build does not ship - the mode is asserted to be refused and "auto" runs in its place."""
    modes = MODES if persistent else ("enqueue", "graph", "auto")
    from locomanipulationrl_amd.lib import EngineError, EpisodeRecord
    torch.manual_seed(seed)
    task = make_task(task_name, N)
    params = [dataclasses.replace(p, **(changes or dict(max_episode=6))) for p in task.engine_params()]
    split = task.split_env() if len(params) == 2 else N
    mani = [int(params[1 if e >= split else 0].mode) == 1 for e in ids]
    kind, packed = make_policy(task)
    log_std = torch.full((12,), -0.3, device="cuda")
    engs = [make_engine(task, N, params) for _ in modes]
    twin = make_engine(task, N, params)
    for e in engs + [twin]:
        if setup: setup(e)
    recs = [guarded_record(e, ids, max_rows, cap) for e in engs + [twin]]
    plans = [make_plan(e, kind, packed, log_std, deterministic=det, episode_record=EpisodeRecord(e) if episode else None, episode_cap=cap if episode else 0,
                       trajectory_record=rec) for e, rec in zip(engs, recs)]
    first_obs(twin)
    for e in engs + [twin]: e.reset_all()          # the recorded steps begin at an episode boundary
    by_hand, hand_epi = recs[-1], EpisodeRecord(twin) if episode else None
    ref_rows, ref_hdr = tr.new_record(len(ids), max_rows)
    if not persistent:
        with pytest.raises(EngineError):
            plans[0].run("persistent")             # refused before anything is launched
    for rep in range(runs):
        for mode, plan in zip(modes, plans):
            plan.run(mode)
        torch.cuda.synchronize()
        for t in range(T):
            r = torch.empty(N, device="cuda"); d = torch.empty(N, dtype=torch.int64, device="cuda")
            twin.step(plans[0].actions[t].contiguous(), None, None, None, r, d)
            by_hand.update(r, d)
            if hand_epi is not None: hand_epi.update(r, d, cap)
            assert torch.equal(r, plans[0].rewards[t]) and torch.equal(d, plans[0].dones[t]), (task_name, rep, t)
            tr.update(ref_rows, ref_hdr, twin.state.cpu().numpy(), twin.cnt.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy(), ids, mani, cap=cap)
        for mode, rec, e in zip(modes + ("lm_trajectory_update",), recs, engs + [twin]):
            got_h, got_r = rec.header.cpu().numpy(), rec.rows.cpu().numpy()
            assert np.array_equal(got_h, ref_hdr), (task_name, mode, rep, got_h.tolist(), ref_hdr.tolist())
            assert tr.same_bits(got_r, ref_rows), (task_name, mode, rep, np.argwhere(got_r.view(np.uint32) != ref_rows.view(np.uint32))[:4].tolist())
            assert guard_intact(rec), (task_name, mode, rep)
            assert same_engines(e, twin), (task_name, mode, rep)
        if episode:
            for plan in plans:
                assert torch.equal(plan.episode_record.record, hand_epi.record)
        for plan in plans: plan.obs[0].copy_(plan.obs[T])
    out = dict(ref_rows=ref_rows, ref_hdr=ref_hdr, recs=recs, plans=plans, engs=engs, twin=twin, mani=mani)
    return out


def close(out):
    for x in out["plans"] + out["engs"] + [out["twin"]]:
        x.close()


# task, envs, tracked envs, does the plan's persistent build ship (the MLP on 64-wide observations: yes; on the 88-wide ones: no)
CASES = [("QuadrupedPoseControl", 40, [0, 15, 16, 39], True), ("QuadrupedManipulatePlate", 48, [0, 17, 47], True),
         ("JointLocomanipulation", 64, [0, 31, 32, 63], True), ("QuadrupedPoseControlCustomController", 48, [0, 20, 47], False)]


# ---------------------------------------------------------------------------------------------- 1. every mode equals the reference
@pytest.mark.parametrize("det", [False, True], ids=["stochastic", "deterministic+episode_record"])
@pytest.mark.parametrize("task_name,N,ids,persistent", CASES)
def test_every_mode_equals_the_reference(task_name, N, ids, persistent, det):
    """Stochastic plans with an uncapped record; deterministic plans with an episode record attached as well and cap = 2 (the combined builds)."""
    out = drive(task_name, N, ids, cap=2 if det else 0, det=det, episode=det, persistent=persistent)
    hdr, rows = out["ref_hdr"], out["ref_rows"]
    # the reference's own tallies: 14 steps, one row each, an episode ended inside the first run and one across the boundary of the runs
    crossing = []
    for k in range(len(ids)):
        ends = np.nonzero(rows[k, :hdr[k, 0], 60])[0]
        assert len(ends) >= 2, (k, ends, hdr[k])
        crossing.append(bool(ends[0] < T <= ends[1]))
        if det:          # cap = 2: the record stops at the second terminal row, inclusive
            assert hdr[k].tolist() == [int(ends[1]) + 1, 2, 0, 0] and not rows[k, hdr[k, 0]:].any()
        else:
            assert hdr[k].tolist() == [2 * T, len(ends), 0, 0]
        # a done row shows the terminal state: progress_buf has not been reset yet
        assert (rows[k, ends, 62] >= 1).all() and (rows[k, :hdr[k, 0], 63] >= 1).all()
    assert any(crossing), crossing          # an episode ended inside the first run and the next one across the boundary of the two runs
    if task_name == "JointLocomanipulation":
        assert out["mani"] == [False, False, True, True]
        tw = out["twin"]
        if not det:          # the last row of an uncapped record is the engine's state now: base on the locomotion side, plate on the other
            assert torch.equal(out["recs"][0].rows[1, 2 * T - 1, 24:31], tw.state[0:7, 31]) and torch.equal(out["recs"][0].rows[2, 2 * T - 1, 24:31], tw.state[37:44, 32])
    close(out)


@pytest.mark.parametrize("det,episode", [(True, False), (False, True)], ids=["deterministic", "stochastic+episode_record"])
def test_the_other_two_combined_builds(det, episode):
    """Deterministic mode alone and an episode record alone next to the trajectory record: the remaining two persistent builds."""
    out = drive("JointLocomanipulation", 64, [0, 31, 32, 63], cap=1, det=det, episode=episode)
    hdr = out["ref_hdr"]
    assert (hdr[:, 1] == 1).all() and (hdr[:, 0] >= 1).all() and (hdr[:, 0] <= 5).all() and (hdr[:, 2] == 0).all()          # cap 1: the reference's recording
    close(out)


# ---------------------------------------------------------------------------------------------- 2. attaching a record changes nothing else
def test_attaching_a_record_changes_nothing_else():
    from locomanipulationrl_amd.lib import TrajectoryRecord
    torch.manual_seed(32)
    N = 40
    task = make_task("QuadrupedPoseControl", N)
    params = [dataclasses.replace(p, max_episode=6) for p in task.engine_params()]
    kind, packed = make_policy(task)
    log_std = torch.full((12,), -0.3, device="cuda")
    for mode in MODES:
        ea, eb = make_engine(task, N, params), make_engine(task, N, params)
        with_rec = make_plan(ea, kind, packed, log_std, trajectory_record=TrajectoryRecord(ea, [0, 15, 16, 39], 2 * T, episode_cap=0))
        without = make_plan(eb, kind, packed, log_std)
        for rep in range(2):
            with_rec.run(mode); without.run(mode); torch.cuda.synchronize()
            for name in BUFFERS:
                assert torch.equal(getattr(with_rec, name), getattr(without, name)), (mode, rep, name)
            assert same_engines(ea, eb) and torch.equal(ea.extras_buf, eb.extras_buf), (mode, rep)
            for p in (with_rec, without): p.obs[0].copy_(p.obs[T])
        assert with_rec.trajectory_record.header[:, 0].tolist() == [2 * T] * 4          # it did record
        for x in (with_rec, without, ea, eb): x.close()


# ---------------------------------------------------------------------------------------------- 3. bounds
@pytest.mark.parametrize("N,ids", [(40, [0, 15, 16, 39]), (40, [33, 39]), (40, [3]), (40, list(range(16, 32))), (72, list(range(71, -1, -1)))],
                         ids=["spread", "ragged_last_block_only", "block0_K1", "K16_one_block", "every_env_K72"])
def test_row_limit_never_writes_past_a_slot(N, ids):
    """max_rows = 3 < the episode's 5 rows: the rest is counted as dropped, and the guard slot behind the rows (same allocation) keeps its bit
    pattern in every mode (drive() checks it after each run).  Blocks of the persistent kernel that own no slot, one slot, 16 slots; K = 72 >
    the 64 ids a wavefront looks at in one go, in descending order, with a ragged last block of 8."""
    out = drive("QuadrupedPoseControl", N, ids, max_rows=3, cap=0)
    hdr = out["ref_hdr"]
    assert (hdr[:, 0] == 3).all() and (hdr[:, 2] == 2 * T - 3).all() and (hdr[:, 1] >= 2).all()
    close(out)


# ---------------------------------------------------------------------------------------------- 4. switching and the C entry points
def test_switching_records_recaptures_the_graph_and_einval_cases():
    from locomanipulationrl_amd.lib import TrajectoryRecord
    torch.manual_seed(33)
    N = 40
    task = make_task("QuadrupedPoseControl", N)
    params = task.engine_params()
    kind, packed = make_policy(task)
    log_std = torch.full((12,), -0.3, device="cuda")
    e = make_engine(task, N, params)
    a, b = TrajectoryRecord(e, [0, 39], 3 * T, episode_cap=0), TrajectoryRecord(e, [16, 5, 39], 3 * T, episode_cap=0)
    plan = make_plan(e, kind, packed, log_std, trajectory_record=a)
    plan.run("graph"); torch.cuda.synchronize()
    assert a.header.tolist() == [[T, int(plan.dones[:, 0].ne(0).sum()), 0, 0], [T, int(plan.dones[:, 39].ne(0).sum()), 0, 0]]
    assert torch.equal(a.rows[:, :T, 59], plan.rewards[:, [0, 39]].T) and torch.equal(a.rows[1, T - 1, 0:12], e.state[13:25, 39])
    rows_a, hdr_a = a.rows.clone(), a.header.clone()
    plan.set_trajectory_record(None); plan.obs[0].copy_(plan.obs[T]); plan.run("graph"); torch.cuda.synchronize()
    assert torch.equal(a.rows, rows_a) and torch.equal(a.header, hdr_a) and plan.trajectory_record is None          # detached: untouched
    plan.set_trajectory_record(b); plan.obs[0].copy_(plan.obs[T]); plan.run("graph"); torch.cuda.synchronize()
    assert torch.equal(a.rows, rows_a) and torch.equal(a.header, hdr_a)
    assert b.header[:, 0].tolist() == [T] * 3 and torch.equal(b.rows[:, :T, 59], plan.rewards[:, [16, 5, 39]].T)          # the graph was re-captured
    assert torch.equal(b.rows[0, T - 1, 0:12], e.state[13:25, 16])
    # ---- LM_EINVAL cases of the setter (host validation: nothing is launched, the attached record stays attached)
    lib = e.lib
    p = lambda t: C.c_void_p(t.data_ptr())
    I = lambda *v: (C.c_int32 * len(v))(*v)
    ok = (p(b.rows), p(b.header), b.max_rows, 0)
    assert lib.lm_rollout_set_trajectory_record(None, I(0), 1, *ok) == -1 and b"lm_rollout_set_trajectory_record" in lib.lm_last_error()
    assert lib.lm_rollout_set_trajectory_record(plan._h, I(0), -1, *ok) == -1
    assert lib.lm_rollout_set_trajectory_record(plan._h, (C.c_int32 * 257)(*range(257)), 257, *ok) == -1
    assert lib.lm_rollout_set_trajectory_record(plan._h, I(0, N), 2, *ok) == -1 and b"outside" in lib.lm_last_error()
    assert lib.lm_rollout_set_trajectory_record(plan._h, I(0, -1), 2, *ok) == -1
    assert lib.lm_rollout_set_trajectory_record(plan._h, I(4, 7, 4), 3, *ok) == -1 and b"repeated" in lib.lm_last_error()
    assert lib.lm_rollout_set_trajectory_record(plan._h, I(0), 1, p(b.rows), p(b.header), 0, 0) == -1
    assert lib.lm_rollout_set_trajectory_record(plan._h, I(0), 1, C.c_void_p(b.rows.data_ptr() + 4), p(b.header), 1, 0) == -1 and b"aligned" in lib.lm_last_error()
    assert lib.lm_rollout_set_trajectory_record(plan._h, I(0), 1, None, p(b.header), 1, 0) == -1
    rew = torch.zeros(N, device="cuda"); dn = torch.zeros(N, dtype=torch.int64, device="cuda")
    upd = lambda h, ids, K, r, d, rows, hdr, m: lib.lm_trajectory_update(h, ids, K, r, d, rows, hdr, m, 0, None)
    assert upd(None, p(b.ids), 3, p(rew), p(dn), p(b.rows), p(b.header), b.max_rows) == -1 and b"lm_trajectory_update" in lib.lm_last_error()
    assert upd(e._h, None, 3, p(rew), p(dn), p(b.rows), p(b.header), b.max_rows) == -1
    assert upd(e._h, p(b.ids), 0, p(rew), p(dn), p(b.rows), p(b.header), b.max_rows) == -1
    assert upd(e._h, p(b.ids), 257, p(rew), p(dn), p(b.rows), p(b.header), b.max_rows) == -1
    assert upd(e._h, p(b.ids), 3, None, p(dn), p(b.rows), p(b.header), b.max_rows) == -1
    assert upd(e._h, p(b.ids), 3, p(rew), None, p(b.rows), p(b.header), b.max_rows) == -1
    assert upd(e._h, p(b.ids), 3, p(rew), p(dn), None, p(b.header), b.max_rows) == -1
    assert upd(e._h, p(b.ids), 3, p(rew), p(dn), p(b.rows), None, b.max_rows) == -1
    assert upd(e._h, p(b.ids), 3, p(rew), p(dn), p(b.rows), p(b.header), 0) == -1
    assert upd(e._h, p(b.ids), 3, p(rew), p(dn), C.c_void_p(b.rows.data_ptr() + 4), p(b.header), b.max_rows) == -1
    if torch.cuda.device_count() > 1:
        with torch.cuda.device(1):
            assert lib.lm_rollout_set_trajectory_record(plan._h, I(0), 1, *ok) == -1 and b"device" in lib.lm_last_error()
            assert upd(e._h, p(b.ids), 3, p(rew), p(dn), p(b.rows), p(b.header), b.max_rows) == -1
    torch.cuda.synchronize()
    assert b.header[:, 0].tolist() == [T] * 3                                       # none of the refused calls touched the record
    # the refused calls left b attached: the next run appends to it
    plan.obs[0].copy_(plan.obs[T]); plan.run("graph"); torch.cuda.synchronize()
    assert b.header[:, 0].tolist() == [2 * T] * 3
    # ---- the kernel skips an id outside [0, N) (the setter refuses such ids; lm_trajectory_update takes device ids it cannot see)
    c = TrajectoryRecord(e, [1, 2, 3], 4, episode_cap=0)
    c.ids.copy_(torch.tensor([1, N + 5, -1], dtype=torch.int32))
    c.update(plan.rewards[T - 1].contiguous(), plan.dones[T - 1].contiguous()); torch.cuda.synchronize()
    assert c.header[:, 0].tolist() == [1, 0, 0] and not c.rows[1:].any() and torch.equal(c.rows[0, 0, 0:12], e.state[13:25, 1])
    plan.close(); e.close()


# ---------------------------------------------------------------------------------------------- 5. families the persistent kernels do not serve
@pytest.mark.parametrize("family", ["randomised", "contact_reporting"])
def test_randomised_and_contact_reporting_engines_record(family):
    """Both record through enqueue and graph ("auto" takes the graph) and equal the reference; "persistent" is refused (drive() asserts it)."""
    if family == "randomised":
        out = drive("QuadrupedPoseControl", 40, [0, 15, 16, 39], changes=dict(dr_enabled=1, max_episode=6), persistent=False)
    else:
        out = drive("QuadrupedPoseControl", 40, [0, 15, 16, 39], setup=lambda e: e.enable_contact_forces(True), persistent=False)
    assert (out["ref_hdr"][:, 0] == 2 * T).all() and (out["ref_hdr"][:, 1] >= 2).all()
    close(out)


# ---------------------------------------------------------------------------------------------- 7. evaluate()
def test_evaluate_returns_the_trajectories_of_the_listed_envs():
    """evaluate(record_envs=[0, N - 1]) fused and step by step: the first recorded episode of each listed env is as long as the episode record
    says, and both paths walk the same trajectory (the same forward kernel), so their rows hold the same bits."""
    import locomanipulationrl_amd as lm
    from locomanipulationrl_amd.policies.mlp_model import SharedMLP
    from locomanipulationrl_amd.train.evaluate import evaluate
    from locomanipulationrl_amd.train.ppo import RunningStandardScaler
    torch.manual_seed(34)
    N = 64
    model = SharedMLP().cuda()
    scaler = RunningStandardScaler(64, "cuda"); scaler.update(torch.randn(256, 64, device="cuda") * 0.5)
    outs = []
    for fused in (True, False):
        env = lm.make_env("QuadrupedPoseControl", num_envs=N, seed=3, overrides={"task": {"sim": {"max_episode_length": 20}}})
        out = evaluate(env, model, scaler, episodes_per_env=1, deterministic=True, fused=fused, return_record=True, record_envs=[0, N - 1])
        traj = out["trajectory"]
        assert traj.max_rows == 20 and traj.episode_cap == 1 and traj.env_ids == [0, N - 1]
        for k, e in enumerate(traj.env_ids):
            eps = traj.episodes(k)
            L = int(out["record"][4, e])
            assert len(eps) == 1 and eps[0]["complete"] and not eps[0]["truncated"] and eps[0]["q"].shape == (L, 12)
            assert traj.header[k].tolist() == [L, 1, 0, 0] and float(eps[0]["progress"][0]) == 1.0 and float(eps[0]["done"][-1]) == 1.0
        outs.append((traj.rows.cpu().numpy(), traj.header.cpu().numpy()))
        env.close()
    assert np.array_equal(outs[0][1], outs[1][1]) and tr.same_bits(outs[0][0], outs[1][0])
