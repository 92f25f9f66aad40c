"""Policy evaluation on the GPU (include/lm_policy.h): deterministic rollouts against a step-by-step loop of the same kernels, the episode
record against the independent numpy reference (tests/episode_reference.py; exact equality - the rule is plain fp32 adds in step order),
both in every rollout mode, and the plumbing around them (switches off change nothing, LM_EINVAL cases, re-capture, randomised engines,
evaluate())."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest
import torch

import episode_reference as er

pytestmark = pytest.mark.gpu

T = 7
MODES = ("enqueue", "graph", "persistent")
BUFFERS = ("obs", "actions", "logp", "values", "rewards", "dones", "extras")


def make_task(task_name, N):
    from locomanipulationrl_amd.utils.config import SimConfig, load_config
    from locomanipulationrl_amd.utils.task_util import task_map
    return task_map()[task_name](name=task_name, sim_config=SimConfig(load_config(task_name, num_envs=N)), env=None)


def make_policy(task, policy, zero=False):
    """(kind, packed parameter block, forward(obs) -> (mean, value)) of a random (or all-zero: mean 0) policy."""
    from locomanipulationrl_amd.lib import POLICY_GNN, POLICY_MLP
    from locomanipulationrl_amd.policies.graph_model import GraphPolicy, gnn_forward_hip, pack_gnn_params
    from locomanipulationrl_amd.policies.mlp_model import SharedMLP, mlp_forward_hip, pack_mlp_params
    nobs = task.engine_params()[0].num_obs
    model = (SharedMLP(num_observations=nobs) if policy == "mlp" else GraphPolicy()).cuda()
    if zero:
        with torch.no_grad():
            for p in model.parameters(): p.zero_()
    if policy == "mlp":
        packed = pack_mlp_params(model, None, None).cuda()
        return POLICY_MLP, packed, lambda o: mlp_forward_hip(o.contiguous(), packed), model
    packed = pack_gnn_params(model.net, model.mean_layer, model.value_layer).cuda()
    return POLICY_GNN, packed, lambda o: gnn_forward_hip(o.contiguous(), packed), model


def make_engine(task, N, params=None, seed=9):
    from locomanipulationrl_amd.lib import Engine
    from locomanipulationrl_amd.model.robot_model import load_model
    return Engine(load_model(task.model_asset), params or task.engine_params(), N, split_env=task.split_env(), seed=seed)


def first_obs(e):
    """The reset step, to have observations to start from."""
    o0 = torch.empty(e.num_envs, e.num_obs, device="cuda"); e.step(torch.zeros(e.num_envs, 12, device="cuda"), None, o0)
    return o0


def make_plan(e, kind, packed, log_std, o0=None, noise_seed=21, **switches):
    from locomanipulationrl_amd.lib import Rollout
    r = Rollout(e, kind, packed, log_std, T, noise_seed=noise_seed, **switches)
    r.obs[0] = first_obs(e) if o0 is None else o0
    return r


def same_engines(a, b):
    return torch.equal(a.state, b.state) and torch.equal(a.cnt, b.cnt) and torch.equal(a.stats_i64, b.stats_i64)


def close(*things):
    for t in things:
        t.close()


LOG_STD = torch.linspace(-1.2, 0.3, 12)          # non-constant


def logp_bound(log_std):
    """Worst-case rounding of twelve fp32 terms (-ls_j - 0.919: a subtraction of magnitude <= |ls_j| + 0.919) and of their sum: each of the at
    most 12 roundings on the way is at most 2^-24 of a partial result bounded by S = sum_j (|ls_j| + 0.919); 12 * 2^-23 * S covers it twice."""
    ls = log_std.double().cpu()
    return float(-(ls + 0.5 * math.log(2.0 * math.pi)).sum()), 12.0 * 2.0 ** -23 * float((ls.abs() + 0.919).sum())


# ---------------------------------------------------------------------------------------------- deterministic == step by step
@pytest.mark.parametrize("task_name,N,policy", [("QuadrupedPoseControl", 40, "mlp"), ("QuadrupedManipulatePlate", 48, "mlp"),
                                                ("JointLocomanipulation", 64, "mlp"), ("QuadrupedPoseControlCustomController", 48, "mlp"),
                                                ("JointLocomanipulationVertical", 64, "gnn")])
def test_deterministic_rollout_equals_step_by_step(task_name, N, policy):
    """actions[t] = the forward's mean bit for bit, in the enqueue, graph and persistent modes, and everything downstream of them equals a
    Python loop of forward -> Engine.step(mean) on a fourth twin; two consecutive runs."""
    torch.manual_seed(5)
    task = make_task(task_name, N)
    kind, packed, fwd, _ = make_policy(task, policy)
    log_std = LOG_STD.cuda()
    engs = [make_engine(task, N) for _ in range(4)]
    plans = [make_plan(e, kind, packed, log_std, deterministic=True) for e in engs[:3]]
    loop = engs[3]; obs = first_obs(loop)
    want, bound = logp_bound(log_std)
    for rep in range(2):
        ref = dict(obs=[obs.clone()], actions=[], values=[], rewards=[], dones=[], extras=[])
        for t in range(T):
            mean, value = fwd(obs)
            o = torch.empty_like(obs); r = torch.empty(N, device="cuda"); d = torch.empty(N, dtype=torch.int64, device="cuda"); ex = torch.empty(13, device="cuda")
            loop.step(mean, None, o, None, r, d, ex)
            ref["actions"].append(mean); ref["values"].append(value.reshape(-1)); ref["rewards"].append(r); ref["dones"].append(d); ref["extras"].append(ex)
            ref["obs"].append(o.clone()); obs = o
        ref["values"].append(fwd(obs)[1].reshape(-1))
        for mode, plan, e in zip(MODES, plans, engs):
            plan.run(mode)
        torch.cuda.synchronize()
        for mode, plan, e in zip(MODES, plans, engs):
            for name in ("obs", "actions", "values", "rewards", "dones", "extras"):
                a, b = getattr(plan, name), torch.stack(ref[name])
                assert torch.equal(a, b), (task_name, mode, rep, name, float((a.float() - b.float()).abs().max()))
            assert same_engines(e, loop), (task_name, mode, rep)
            lp = plan.logp
            assert bool((lp == lp[0, 0]).all()), (mode, rep)                       # the same number for every env and step
            assert abs(float(lp[0, 0]) - want) <= bound, (float(lp[0, 0]), want, bound)
            assert torch.equal(lp, plans[0].logp)
            plan.obs[0].copy_(plan.obs[T])
    close(*plans, *engs)


def test_deterministic_actions_survive_an_overflowing_exp_log_std():
    """log_std = +100: exp overflows to inf, and inf * 0 would be a NaN; the mean itself is written."""
    torch.manual_seed(6)
    N = 40
    task = make_task("QuadrupedPoseControl", N)
    kind, packed, fwd, _ = make_policy(task, "mlp")
    log_std = torch.full((12,), 100.0, device="cuda")
    engs = [make_engine(task, N) for _ in range(3)]
    plans = [make_plan(e, kind, packed, log_std, deterministic=True) for e in engs]
    for mode, plan in zip(MODES, plans):
        plan.run(mode)
    torch.cuda.synchronize()
    for mode, plan in zip(MODES, plans):
        assert torch.isfinite(plan.actions).all() and torch.isfinite(plan.obs).all() and torch.isfinite(plan.logp).all(), mode
        for t in range(T):
            assert torch.equal(plan.actions[t], fwd(plan.obs[t])[0]), (mode, t)
        assert torch.equal(plan.actions, plans[0].actions) and torch.equal(plan.logp, plans[0].logp)
    close(*plans, *engs)


# ---------------------------------------------------------------------------------------------- switches off change nothing
@pytest.mark.parametrize("mode", ["graph", "persistent"])
def test_a_record_attached_to_a_stochastic_plan_changes_no_buffer(mode):
    from locomanipulationrl_amd.lib import EpisodeRecord
    torch.manual_seed(7)
    N = 40
    task = make_task("QuadrupedPoseControl", N)
    kind, packed, _, _ = make_policy(task, "mlp")
    log_std = torch.full((12,), -0.3, device="cuda")
    ea, eb = make_engine(task, N), make_engine(task, N)
    with_rec = make_plan(ea, kind, packed, log_std, episode_record=EpisodeRecord(ea)); without = make_plan(eb, kind, packed, log_std)
    for rep in range(2):
        with_rec.run(mode); without.run(mode); torch.cuda.synchronize()
        for name in BUFFERS:
            assert torch.equal(getattr(with_rec, name), getattr(without, name)), (mode, rep, name)
        assert same_engines(ea, eb) and torch.equal(ea.extras_buf, eb.extras_buf)
        for p in (with_rec, without): p.obs[0].copy_(p.obs[T])
    assert float(with_rec.episode_record.record[1].sum()) + float(with_rec.episode_record.record[4].sum()) == 2 * T * N      # it did record
    close(with_rec, without, ea, eb)


@pytest.mark.parametrize("mode", ["graph", "persistent"])
def test_deterministic_switched_on_and_off_again_equals_a_plan_that_never_had_it(mode):
    torch.manual_seed(8)
    N = 40
    task = make_task("QuadrupedPoseControl", N)
    kind, packed, _, _ = make_policy(task, "mlp")
    log_std = torch.full((12,), -0.3, device="cuda")
    ea, eb = make_engine(task, N), make_engine(task, N)
    flipped = make_plan(ea, kind, packed, log_std); never = make_plan(eb, kind, packed, log_std)
    flipped.run(mode); never.run(mode)                          # (captures the graph before the switch is touched)
    flipped.set_deterministic(True); flipped.set_deterministic(False)
    for p in (flipped, never): p.obs[0].copy_(p.obs[T])
    flipped.run(mode); never.run(mode); torch.cuda.synchronize()
    for name in BUFFERS:
        assert torch.equal(getattr(flipped, name), getattr(never, name)), (mode, name)
    assert same_engines(ea, eb)
    close(flipped, never, ea, eb)


# ---------------------------------------------------------------------------------------------- record == reference
def _blocks(task, per_block):
    return [dataclasses.replace(p, **ch) for p, ch in zip(task.engine_params(), per_block)]


# name -> (task, envs, per-block parameter changes, zero policy?, log_std, [(env slice, intended outcome row)])
RECORD_CASES = {
    "failures": ("QuadrupedPoseControl", 40, [dict(h_base=1.0)], True, 0.0, [(slice(None), er.FAILURE)]),
    "timeouts": ("QuadrupedPoseControl", 40, [dict(max_episode=6)], True, 0.0, [(slice(None), er.TIMEOUT)]),
    "goals": ("QuadrupedPoseControl", 40, [dict(succ_thresh=4.0, max_consec=3)], True, 0.0, [(slice(None), er.GOAL)]),
    "cotrain": ("JointLocomanipulation", 64, [dict(max_episode=6), dict(succ_thresh=4.0, max_consec=3)], True, 0.0,
                [(slice(0, 32), er.TIMEOUT), (slice(32, 64), er.GOAL)]),
    "stochastic": ("QuadrupedPoseControl", 40, [dict(max_episode=10)], False, -0.3, None),
}


@pytest.mark.parametrize("case", list(RECORD_CASES))
def test_episode_record_equals_reference_in_every_mode(case):
    """Three runs of T = 7 (episodes of length 5 cross the rollout boundaries).  The streams are the rollout's own rewards / dones; the goal
    flags come from a step-by-step twin that replays the rollout's actions and reads the terms view it asked for before stepping.  The same
    twin drives lm_episode_update by hand after each Engine.step."""
    from locomanipulationrl_amd.lib import EpisodeRecord
    torch.manual_seed(11)
    task_name, N, changes, zero, ls, intended = RECORD_CASES[case]
    task = make_task(task_name, N)
    params = _blocks(task, changes)
    M = np.concatenate([np.full(N // len(params), p.max_episode) for p in params])
    kind, packed, _, _ = make_policy(task, "mlp", zero=zero)
    log_std = torch.full((12,), ls, device="cuda")
    engs = [make_engine(task, N, params) for _ in MODES]
    recs = [EpisodeRecord(e) for e in engs]
    plans = [make_plan(e, kind, packed, log_std, deterministic=zero, episode_record=rec) for e, rec in zip(engs, recs)]
    twin = make_engine(task, N, params); _ = twin.terms; first_obs(twin)
    for e in engs + [twin]: e.reset_all()          # the recorded steps begin at an episode boundary: a length is counted from the reset step
    by_hand = EpisodeRecord(twin)
    assert by_hand.split == (32 if case == "cotrain" else None)
    ref = er.new_record(N)
    wins0 = int(twin.stats_i64[0])
    for rep in range(3):
        for mode, plan in zip(MODES, plans):
            plan.run(mode)
        torch.cuda.synchronize()
        goals = []
        for t in range(T):
            r = torch.empty(N, device="cuda"); d = torch.empty(N, dtype=torch.int64, device="cuda")
            twin.step(plans[0].actions[t].contiguous(), None, None, None, r, d)
            by_hand.update(r, d)
            assert torch.equal(r, plans[0].rewards[t]) and torch.equal(d, plans[0].dones[t])
            goals.append(twin.terms[7].cpu().numpy().copy())
        er.update(ref, plans[0].rewards.cpu().numpy(), plans[0].dones.cpu().numpy(), np.stack(goals), M)
        for mode, rec in zip(MODES + ("lm_episode_update",), recs + [by_hand]):
            got = rec.record.cpu().numpy()
            assert np.array_equal(got, ref), (case, mode, rep, [int(q) for q in np.nonzero((got != ref).any(1))[0]])
        for plan in plans: plan.obs[0].copy_(plan.obs[T])
    # the reference's own tallies: the streams did contain what the case is about
    episodes = ref[er.EPISODES]
    if intended is None:
        assert (episodes >= 1).all(), episodes
    else:
        for sl, row in intended:
            assert episodes[sl].sum() > 0 and ref[row, sl].sum() >= 0.9 * episodes[sl].sum(), (case, er.tallies(ref[:, sl]))
    # goals summed over the envs = the growth of num_successes over the same steps (far fewer resets than a success window holds)
    assert int(ref[er.GOAL].sum()) == int(twin.stats_i64[0]) - wins0
    s = recs[0].summary()
    assert s["episodes"] == int(episodes.sum()) and abs(s["success_rate"] + s["timeout_rate"] + s["failure_rate"] - 1.0) < 1e-12
    if case == "cotrain":
        assert s["loco"]["timeout_rate"] >= 0.9 and s["mani"]["success_rate"] >= 0.9 and s["loco"]["episodes"] + s["mani"]["episodes"] == s["episodes"]
    close(*plans, *engs, twin)


def test_episode_cap_freezes_every_env_after_its_first_episodes():
    """cap = 2 on the timeout case (an episode every 5 steps, 21 steps): every env's row 2 ends at exactly 2 and its rows are the reference's
    after its second episode, in every mode."""
    from locomanipulationrl_amd.lib import EpisodeRecord
    N = 40
    task = make_task("QuadrupedPoseControl", N)
    params = _blocks(task, [dict(max_episode=6)])
    kind, packed, _, _ = make_policy(task, "mlp", zero=True)
    log_std = torch.zeros(12, device="cuda")
    engs = [make_engine(task, N, params) for _ in MODES]
    recs = [EpisodeRecord(e) for e in engs]
    plans = [make_plan(e, kind, packed, log_std, deterministic=True, episode_record=rec, episode_cap=2) for e, rec in zip(engs, recs)]
    twin = make_engine(task, N, params); _ = twin.terms; first_obs(twin)
    for e in engs + [twin]: e.reset_all()
    ref = er.new_record(N)
    for rep in range(3):
        for mode, plan in zip(MODES, plans):
            plan.run(mode)
        torch.cuda.synchronize()
        goals = []
        for t in range(T):
            twin.step(plans[0].actions[t].contiguous()); goals.append(twin.terms[7].cpu().numpy().copy())
        er.update(ref, plans[0].rewards.cpu().numpy(), plans[0].dones.cpu().numpy(), np.stack(goals), 6, cap=2)
        for plan in plans: plan.obs[0].copy_(plan.obs[T])
    uncapped = int(sum(int(p.dones.sum()) for p in plans[:1]))
    assert (ref[er.EPISODES] == 2).all() and (ref[er.RUN_LENGTH] == 0).all() and (ref[er.SUM_LENGTH] == 10).all() and uncapped > 0
    for mode, rec in zip(MODES, recs):
        assert np.array_equal(rec.record.cpu().numpy(), ref), mode
    close(*plans, *engs, twin)


# ---------------------------------------------------------------------------------------------- plumbing
def test_einval_cases_and_recapture_after_a_switch():
    from locomanipulationrl_amd.lib import EngineError, EpisodeRecord
    torch.manual_seed(12)
    N = 40
    task = make_task("QuadrupedPoseControl", N)
    kind, packed, _, _ = make_policy(task, "mlp")
    log_std = LOG_STD.cuda()
    ea, eb = make_engine(task, N), make_engine(task, N)
    lib = ea.lib
    rec = EpisodeRecord(ea)
    rew = torch.zeros(N, device="cuda"); dn = torch.zeros(N, dtype=torch.int64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.lm_rollout_set_deterministic(None, 1) == -1 and lib.lm_rollout_set_episode_record(None, p(rec.record), 0) == -1
    assert lib.lm_episode_update(None, p(rew), p(dn), p(rec.record), 0, None) == -1
    assert lib.lm_episode_update(ea._h, None, p(dn), p(rec.record), 0, None) == -1 and b"lm_episode_update" in lib.lm_last_error()
    assert lib.lm_episode_update(ea._h, p(rew), None, p(rec.record), 0, None) == -1
    assert lib.lm_episode_update(ea._h, p(rew), p(dn), None, 0, None) == -1
    # a plan created (and captured) before the switches were flipped re-captures and runs: equal to a plan created with them
    late = make_plan(ea, kind, packed, log_std); born = make_plan(eb, kind, packed, log_std, deterministic=True, episode_record=EpisodeRecord(eb))
    o0 = late.obs[0].clone()
    late.run("graph"); torch.cuda.synchronize()
    ea.load_state_dict(eb.state_dict()); late.obs[0].copy_(o0)          # back to the start: eb has not run yet
    late.set_deterministic(True); late.set_episode_record(rec)
    if torch.cuda.device_count() > 1:                                       # a calling thread on another device than the engine's
        with torch.cuda.device(1):
            assert lib.lm_rollout_set_deterministic(late._h, 1) == -1 and b"device" in lib.lm_last_error()
            assert lib.lm_rollout_set_episode_record(late._h, p(rec.record), 0) == -1
            assert lib.lm_episode_update(ea._h, p(rew), p(dn), p(rec.record), 0, None) == -1
    late.run("graph"); born.run("graph"); torch.cuda.synchronize()
    for name in BUFFERS:
        assert torch.equal(getattr(late, name), getattr(born, name)), name
    assert torch.equal(rec.record, born.episode_record.record) and float(rec.record[1].sum() + rec.record[4].sum()) == T * N
    # recording off again: the record stops moving
    late.set_episode_record(None); before = rec.record.clone(); late.obs[0].copy_(late.obs[T]); late.run("graph"); torch.cuda.synchronize()
    assert torch.equal(rec.record, before)
    close(late, born, ea, eb)


def test_randomised_engine_graph_equals_enqueue_with_both_switches_on():
    from locomanipulationrl_amd.lib import EngineError, EpisodeRecord
    torch.manual_seed(13)
    N = 40
    task = make_task("QuadrupedPoseControl", N)
    params = _blocks(task, [dict(dr_enabled=1, max_episode=6)])
    kind, packed, _, _ = make_policy(task, "mlp")
    log_std = LOG_STD.cuda()
    engs = [make_engine(task, N, params) for _ in range(2)]
    plans = [make_plan(e, kind, packed, log_std, deterministic=True, episode_record=EpisodeRecord(e)) for e in engs]
    for rep in range(2):
        plans[0].run("enqueue"); plans[1].run("graph"); torch.cuda.synchronize()
        for name in BUFFERS:
            assert torch.equal(getattr(plans[0], name), getattr(plans[1], name)), (rep, name)
        assert torch.equal(plans[0].episode_record.record, plans[1].episode_record.record) and same_engines(*engs)
        for p in plans: p.obs[0].copy_(p.obs[T])
    assert float(plans[0].episode_record.record[2].sum()) > 0
    with pytest.raises(EngineError):
        plans[0].run("persistent")
    plans[0].run("auto"); torch.cuda.synchronize()          # takes the graph
    close(*plans, *engs)


@pytest.mark.parametrize("task_name,N,policy", [("QuadrupedPoseControlCustomController", 48, "mlp"), ("JointLocomanipulationVertical", 64, "gnn")])
def test_recording_plans_without_a_persistent_build_take_the_graph(task_name, N, policy):
    """The persistent kernels keep the record only on the 64-wide MLP (the other recording builds would need scratch memory): on the 88-wide MLP
    and on the GNN a plan with a record attached is refused in persistent mode (-1), "auto" runs it as the graph - identical to the enqueue mode -
    and with the record detached persistent runs again."""
    from locomanipulationrl_amd.lib import EngineError, EpisodeRecord
    torch.manual_seed(15)
    task = make_task(task_name, N)
    params = _blocks(task, [dict(max_episode=6)] * len(task.engine_params()))
    kind, packed, _, _ = make_policy(task, policy)
    log_std = LOG_STD.cuda()
    engs = [make_engine(task, N, params) for _ in range(2)]
    plans = [make_plan(e, kind, packed, log_std, deterministic=True, episode_record=EpisodeRecord(e)) for e in engs]
    with pytest.raises(EngineError):
        plans[1].run("persistent")
    for rep in range(2):
        plans[0].run("enqueue"); plans[1].run("auto"); torch.cuda.synchronize()
        for name in BUFFERS:
            assert torch.equal(getattr(plans[0], name), getattr(plans[1], name)), (rep, name)
        assert torch.equal(plans[0].episode_record.record, plans[1].episode_record.record) and same_engines(*engs)
        for p in plans: p.obs[0].copy_(p.obs[T])
    assert int(plans[0].episode_record.record[er.EPISODES].sum()) >= N          # max_episode 6, 14 steps: every env completed an episode
    rec = plans[1].episode_record; before = rec.record.clone()
    plans[1].set_episode_record(None); plans[0].set_episode_record(None)
    plans[0].run("enqueue"); plans[1].run("persistent"); torch.cuda.synchronize()
    for name in BUFFERS:
        assert torch.equal(getattr(plans[0], name), getattr(plans[1], name)), name
    assert torch.equal(rec.record, before)
    close(*plans, *engs)


def test_evaluate_fused_equals_step_by_step():
    """evaluate() on twin 64-env environments with the same policy, deterministic: the fused rollouts and the Python loop walk the same
    trajectory (the same forward kernel), so episodes, outcome counts and the per-env fp32 rows are equal.  The host reduction is the only
    step that is not the same arithmetic as a reference sum: mean_return is a float64 sum of N = 64 rows (each exact in float64) and one
    division, so it lies within (N - 1) * 2^-53 * sum |row 3| / episodes + 2^-53 |mean| of the exactly rounded value (math.fsum)."""
    import locomanipulationrl_amd as lm
    from locomanipulationrl_amd.policies.mlp_model import SharedMLP
    from locomanipulationrl_amd.train.evaluate import evaluate
    from locomanipulationrl_amd.train.ppo import RunningStandardScaler
    torch.manual_seed(14)
    N = 64
    model = SharedMLP().cuda()
    scaler = RunningStandardScaler(64, "cuda"); scaler.update(torch.randn(256, 64, device="cuda") * 0.5)
    outs = []
    for fused in (True, False):
        env = lm.make_env("QuadrupedPoseControl", num_envs=N, seed=3, overrides={"task": {"sim": {"max_episode_length": 20}}})
        outs.append(evaluate(env, model, scaler, episodes_per_env=2, deterministic=True, fused=fused, return_record=True))
        env.close()
    a, b = outs
    for k in ("episodes", "goals", "timeouts", "failures", "envs_short"):
        assert a[k] == b[k], (k, a[k], b[k])
    assert a["episodes"] == 2 * N and a["envs_short"] == 0 and a["goals"] + a["timeouts"] + a["failures"] == a["episodes"]
    assert torch.equal(a["record"], b["record"])
    assert a["steps"] % 48 == 0 and b["steps"] <= 2 * 20
    row3 = a["record"][er.SUM_RETURN].double().tolist()
    exact = math.fsum(row3) / a["episodes"]
    bound = (N - 1) * 2.0 ** -53 * math.fsum(abs(x) for x in row3) / a["episodes"] + 2.0 ** -53 * abs(exact)
    for out in (a, b):
        assert abs(out["mean_return"] - exact) <= bound, (out["mean_return"], exact, bound)
