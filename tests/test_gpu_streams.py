"""Every launch entry point of include/lm_engine.h and include/lm_policy.h on a caller's stream and inside a caller's graph.

"The stream is the caller's" (lm_engine.h).  The rest of the suite runs on torch's default stream, the legacy null stream, which is ordered against
everything: there a launch that drops its stream argument, a helper kernel on stream 0 or a blocking copy that overtakes queued work computes the
right bits all the same.  Here every call runs on a non-blocking side stream S (a torch.cuda.Stream() that the `rig` fixture has seen run beside
the default stream, see there) behind a device-side delay:

  baseline        the sequence on the default stream, fresh objects, fixed seeds; outputs and internal state copied to the host
  run under test  a second, identical set of objects.  Every buffer the call reads first holds a POISON (valid values of a second draw).  On S:
                  the delay, the producer (an on-device copy of the real inputs into those buffers; where the input is engine state, an
                  engine.step that changes it), the call, a consumer copy of every output.  Then, on the default stream and before any
                  synchronisation, a clone of one poisoned buffer; then S.synchronize()
  asserted        the consumer copies and the internal state equal the baseline's bit for bit; the clone still shows the poison ("window
                  closed" otherwise: the call was not enqueued while the delay held the producer back, so the case proved nothing)

A launch that escaped S would have read the poison; test_control_the_poison_discriminates shows that this changes the bits.  No tolerance appears in
this module: the criterion is equality of bits.

The delay is torch.cuda._sleep, calibrated against device events when the module starts.  Measured on the MI355X: enqueueing the longest case, a
whole PPO iteration (test_trainer_iteration_on_a_callers_stream, which prints the figure), takes 0.34 - 0.39 ms of host time (ENQUEUE_MS = 0.4);
the delay DELAY_MS = 50 ms is 125 times that (at least 20 times is asked for, 250 ms is the cap) and leaves room for the one case that also
captures and instantiates a graph while it enqueues.  It is a bounded spin, not a hang.

On the commit before this module the six setter cases failed (every one a mismatch: step(a1) ran with the rows of the setter that was called
after it) and everything else passed; lm_set_env_params / lm_clear_env_params now wait for the device first.

The setter cases pin the contract of lm_set_env_params / lm_clear_env_params against work in flight, the graph cases the two claims the header
makes about a hipGraph the caller captured around lm_step.  COVERED maps every prototype with a `void* stream` parameter to its cases;
tests/test_streams_covered.py (no GPU) fails when an entry point is added without one."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from locomanipulationrl_amd.engine_config import DR_BASE_FORCE, DR_CHANNELS, DR_DISTRIBUTIONS, DR_GRAVITY, DR_OPERATIONS, DRChannel, loco_cc_params, loco_params

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, T, B = 40, 3, 37          # two full wavefronts and a ragged one of 8 envs; rollout length; batch of the gradient kernels
ENQUEUE_MS = 0.4             # host time to enqueue the trainer iteration, measured on the MI355X (printed by the trainer case)
DELAY_MS = 50.0              # >= 20 x ENQUEUE_MS, <= 250

# entry point (every prototype of the two headers with a `void* stream` parameter) -> the cases that run it on a caller's stream
COVERED = {
    "lm_step": ["step_w1", "step_h2", "step_h3", "step_w2", "step_pd", "step_dr", "step_dr_pd", "step_contact", "step_env_params",
                "test_setters_against_work_in_flight", "test_caller_graph_replays_equal_eager", "test_caller_graph_sees_new_env_params"],
    "lm_post_physics": ["post_physics"],
    "lm_reset_all": ["reset_all"],
    "lm_task_eval": ["task_eval"],
    "lm_apply_resets": ["apply_resets"],
    "lm_substeps": ["substeps", "substeps_contact"],
    "lm_forward_kinematics": ["forward_kinematics"],
    "lm_debug_dynamics": ["debug_dynamics"],
    "lm_gnn_forward": ["gnn_forward"],
    "lm_mlp_forward": ["mlp_forward"],
    "lm_mlp_forward_obs": ["mlp_forward_obs_64", "mlp_forward_obs_88", "test_caller_graph_replays_equal_eager"],
    "lm_sample_actions": ["sample_actions", "test_caller_graph_replays_equal_eager"],
    "lm_rollout_run": ["rollout_mlp_enqueue", "rollout_mlp_graph", "rollout_mlp_persistent", "rollout_gnn_enqueue", "rollout_gnn_graph",
                       "rollout_gnn_persistent", "rollout_records_graph", "test_trainer_iteration_on_a_callers_stream"],
    "lm_episode_update": ["episode_update", "rollout_records_graph", "test_caller_graph_replays_equal_eager"],
    "lm_trajectory_update": ["trajectory_update", "rollout_records_graph"],
    "lm_replay_update": ["replay_update"],
    "lm_mlp_ppo_grad": ["mlp_ppo_grad_64", "mlp_ppo_grad_88", "test_trainer_iteration_on_a_callers_stream"],
    "lm_gae": ["gae", "test_trainer_iteration_on_a_callers_stream"],
    "lm_gnn_ppo_grad": ["gnn_ppo_grad"],
    "lm_optim_state_init": ["optim_state_init"],
    "lm_adam_clip_step": ["adam_clip_step", "test_trainer_iteration_on_a_callers_stream"],
    "lm_kl_adaptive_lr": ["kl_adaptive_lr", "test_trainer_iteration_on_a_callers_stream"],
    "lm_mlp_pack_params": ["mlp_pack_params", "test_trainer_iteration_on_a_callers_stream"],
    "lm_gnn_pack_params": ["gnn_pack_params"],
    "lm_ppo_batch_stats": ["batch_stats", "test_trainer_iteration_on_a_callers_stream"],
    "lm_ppo_batch_apply": ["batch_apply", "test_trainer_iteration_on_a_callers_stream"],
}

ENV_KEYS = ("LM_H2_MAX_ENVS", "LM_H3_MAX_ENVS", "LM_W2_MIN_ENVS")
FORCE = {"w1": {"LM_H2_MAX_ENVS": "0"}, "h2": {"LM_H2_MAX_ENVS": "1000000"}, "h3": {"LM_H3_MAX_ENVS": "1000000"}, "w2": {"LM_W2_MIN_ENVS": "1"}}


# ------------------------------------------------------------------------------------------------ harness
def bits(x):
    """A host copy whose equality is equality of bits (NaN payloads and the sign of zero included)."""
    x = x.detach().cpu().contiguous()
    return x.view(torch.int32) if x.dtype == torch.float32 else x.view(torch.int64) if x.dtype == torch.float64 else x


def assert_same_bits(got, want, tag):
    assert len(got) == len(want), (tag, len(got), len(want))
    for k, (x, y) in enumerate(zip(got, want)):
        assert x.dtype == y.dtype and x.shape == y.shape, (tag, k, x.dtype, y.dtype, tuple(x.shape), tuple(y.shape))
        assert torch.equal(x, y), f"mismatch: {tag}, item {k} of the outputs + internal state differs from the default-stream baseline in {int((x != y).sum())} of {x.numel()} words"


def draws(seed, *shapes, lo=-1.0, hi=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [torch.rand(*s, device=DEV, generator=g) * (hi - lo) + lo for s in shapes]


class Case:
    """bufs: [(buffer, real, poison)], the buffer holding the poison; producer: what else runs before the call (an engine.step, on the same stream);
    call: the call under test, returns its outputs; state: the internal state to compare; after(S): more work once the consumer copies are
    enqueued (S None: the baseline), returns more outputs; keep: objects closed, in order, when the case is done."""

    def __init__(self, bufs, call, state=None, producer=None, after=None, keep=()):
        self.bufs, self.call, self.state, self.producer, self.after, self.keep = bufs, call, state or (lambda: []), producer, after, list(keep)

    def close(self):
        torch.cuda.synchronize()
        for k in self.keep:
            k.close()


def run_baseline(c):
    for buf, real, _ in c.bufs:
        buf.copy_(real)
    if c.producer: c.producer()
    out = [o.clone() for o in c.call()]
    if c.after: out += c.after(None)
    torch.cuda.synchronize()
    res = [bits(o) for o in out] + [bits(s) for s in c.state()]
    c.close()
    return res


def run_on_stream(c, rig):
    """-> (outputs + internal state, window open)."""
    S = rig.S
    assert S.cuda_stream != 0 and S != torch.cuda.default_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        rig.delay()
        for buf, real, _ in c.bufs:
            buf.copy_(real)
        if c.producer: c.producer()
        out = [torch.empty_like(o).copy_(o) for o in c.call()]
        if c.after: out += c.after(S)
    probe = c.bufs[0][0].clone()          # the default stream, before any synchronisation
    S.synchronize()
    torch.cuda.synchronize()
    window = torch.equal(bits(probe), bits(c.bufs[0][2]))
    res = [bits(o) for o in out] + [bits(s) for s in c.state()]
    c.close()
    return res, window


WINDOW_CLOSED = ("window closed: the default stream no longer saw the poison after the case was enqueued - the delay did not hold the producer back for "
                 "that long (or something in the case waited for the device), so the run proves nothing about its launches")


class Rig:
    """S: a side stream whose work runs concurrently with the default stream's; delay(): a spin of DELAY_MS on the current stream."""

    def __init__(self, S, delay):
        self.S, self.delay = S, delay


@pytest.fixture(scope="module")
def rig():
    """torch.cuda._sleep counts device clock ticks: calibrated here against events.  The side stream is chosen, not assumed: the runtime maps its
    streams onto a few hardware queues, and a side stream that shares the default stream's queue runs in order with it - behind such a stream a
    launch that escaped to stream 0 would wait for the delay like everything else and read the real inputs.  So a stream is kept only after a
    default-stream kernel has been seen to finish while a short spin on it was still running."""
    from locomanipulationrl_amd.lib import build_library
    build_library()
    assert 20.0 * ENQUEUE_MS <= DELAY_MS <= 250.0
    torch.cuda._sleep(1000); torch.cuda.synchronize()
    ticks, ms = 200_000, 0.0
    for _ in range(6):          # until the spin is long enough to time
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); torch.cuda._sleep(ticks); e1.record(); e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 2.0: break
        ticks *= 8
    assert ms >= 2.0, ("torch.cuda._sleep could not be calibrated", ticks, ms)
    per_ms = ticks / ms
    x = torch.zeros(64, device=DEV)
    tried = []
    for _ in range(32):          # torch hands out its pool of side streams in turn
        S = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(S):
            torch.cuda._sleep(int(10 * per_ms))
            spun = S.record_event()
        x.clone()
        done = torch.cuda.default_stream().record_event()
        done.synchronize()
        concurrent = not spun.query()
        S.synchronize()
        tried.append(concurrent)
        if concurrent: break
    assert tried[-1], "no side stream runs concurrently with the default stream: the cases of this module cannot tell a launch on stream 0 from one on S"
    n = int(per_ms * DELAY_MS)
    print(f"[streams] torch.cuda._sleep: {per_ms:.0f} ticks per ms, the delay of {DELAY_MS} ms is {n} ticks; side stream {len(tried)} of the pool runs beside the default stream")
    return Rig(S, lambda: torch.cuda._sleep(n))


# ------------------------------------------------------------------------------------------------ engines
def outs(n, num_obs=64):
    return [torch.zeros(n, num_obs, device=DEV), torch.zeros(n, 93, device=DEV), torch.zeros(n, device=DEV),
            torch.zeros(n, dtype=torch.int64, device=DEV), torch.zeros(13, device=DEV)]      # obs, states, rew, resets, extras


def engine(rm, mp, eps, variant="w1", n=N, seed=5, **kw):
    from locomanipulationrl_amd.lib import Engine
    for k in ENV_KEYS: mp.delenv(k, raising=False)
    for k, v in FORCE[variant].items(): mp.setenv(k, v)
    e = Engine(rm, eps, n, seed=seed, **kw)
    for k in FORCE[variant]: mp.delenv(k)
    return e


def internal(e):
    s = [e.state, e.cnt, e.rew_buf, e.extras_buf, e.stats_i64, e._stats_i32, e.dr_cnt]
    if e.params[0].dr_enabled:
        s += [e.dr_phys, e.dr_mu, e.dr_mass, e.dr_actuator]
    if e.env_params_enabled:
        s.append(e._env_table())
    if e.lib.lm_ptr(e._h, 12):          # LM_PTR_CONTACT
        s.append(e._contact_record())
    return s


def dr_channels():
    """Channels that draw in every step (interval 1), so that the randomisation counters and records move."""
    dr = [DRChannel() for _ in range(DR_CHANNELS)]
    dr[DR_GRAVITY] = DRChannel(enabled=1, operation=DR_OPERATIONS["additive"], distribution=DR_DISTRIBUTIONS["gaussian"], interval=1, p0=[0.0, 0.0, 0.0], p1=[0.3, 0.3, 0.5])
    dr[DR_BASE_FORCE] = DRChannel(enabled=1, operation=DR_OPERATIONS["direct"], distribution=DR_DISTRIBUTIONS["uniform"], interval=1, p0=[-0.5] * 3, p1=[0.5] * 3)
    return dr


def warmed(e, seed=11):
    """One step on the default stream (it resets every env); -> its output buffers and three action draws: the next real one, the poison, a spare."""
    a0, a1, ap, a2 = draws(seed, (N, 12), (N, 12), (N, 12), (N, 12))
    o = outs(N, e.num_obs)
    e.step(a0, None, *o)
    torch.cuda.synchronize()
    return o, a1, ap, a2


CASES = {}


def case(cid):
    def reg(f):
        assert cid not in CASES
        CASES[cid] = f
        return f
    return reg


def step_case(cid, make, variant="w1"):
    @case(cid)
    def build(rm, mp):
        e = make(rm, mp)
        assert e.step_variant == variant
        o, a1, ap, _ = warmed(e)
        buf = ap.clone()

        def call():
            e.step(buf, None, *o)
            return o
        return Case([(buf, a1, ap)], call, lambda: internal(e), keep=[e])


for _v in ("w1", "h2", "h3", "w2"):
    step_case("step_" + _v, lambda rm, mp, v=_v: engine(rm, mp, [loco_params()], v), _v)
step_case("step_pd", lambda rm, mp: engine(rm, mp, [loco_cc_params()]))
step_case("step_dr", lambda rm, mp: engine(rm, mp, [loco_params(dr_enabled=1, dr=dr_channels())]))
step_case("step_dr_pd", lambda rm, mp: engine(rm, mp, [loco_cc_params(dr_enabled=1, dr=dr_channels())]))


def _contact_engine(rm, mp):
    e = engine(rm, mp, [loco_params()]); e.enable_contact_forces()
    return e


def _env_params_engine(rm, mp):
    e = engine(rm, mp, [loco_params(dr_enabled=1)]); e.enable_env_params()
    e.set_env_params(mu=np.linspace(0.2, 1.2, N).astype(np.float32))
    return e


step_case("step_contact", _contact_engine)
step_case("step_env_params", _env_params_engine)


def action_case(cid, call_of, make=lambda rm, mp: engine(rm, mp, [loco_params()]), prepare=None):
    """Cases whose only buffer is an action block: call_of(e, buf, o) -> (producer or None, call)."""
    @case(cid)
    def build(rm, mp):
        e = make(rm, mp)
        o, a1, ap, _ = warmed(e)
        if prepare: prepare(e)
        buf = ap.clone()
        producer, call = call_of(e, buf, o)
        return Case([(buf, a1, ap)], call, lambda: internal(e), producer=producer, keep=[e])


def _after(f):
    """call_of for an entry point that reads engine state: the producer is a step on the same stream."""
    return lambda e, buf, o: ((lambda: e.step(buf, None, *o)), (lambda: o + list(f(e, o) or [])))


action_case("post_physics", lambda e, buf, o: (None, lambda: (e.post_physics(buf, *o), o)[1]))
action_case("substeps", lambda e, buf, o: (None, lambda: (e.substeps(buf, 2), [])[1]))
action_case("substeps_contact", lambda e, buf, o: (None, lambda: (e.substeps(buf, 2), [])[1]), make=_contact_engine)
action_case("reset_all", _after(lambda e, o: e.reset_all()))
action_case("forward_kinematics", _after(lambda e, o: e.forward_kinematics()))
action_case("debug_dynamics", _after(lambda e, o: e.debug_dynamics()))


@case("apply_resets")
def _apply_resets(rm, mp):
    e = engine(rm, mp, [loco_params()])
    warmed(e); e.reset_all()
    real, poison = draws(21, (N, 3), (N, 3), lo=0.0)
    buf = poison.clone()
    return Case([(buf, real, poison)], lambda: (e.apply_resets(buf), [])[1], lambda: internal(e), keep=[e])


@case("task_eval")
def _task_eval(rm, mp):
    """The read-back of the engine's own state after a step (layout of the oracle: q, qd, qdd, free body, tips, knees; no torque)."""
    e = engine(rm, mp, [loco_params()])
    o, a1, ap, _ = warmed(e)
    tips, knees = e.forward_kinematics()
    rb = torch.zeros(N, 99, device=DEV)
    rb[:, 0:12] = e.state[13:25].T; rb[:, 12:24] = e.state[25:37].T; rb[:, 36:49] = e.state[0:13].T
    rb[:, 49:61] = tips.reshape(N, 12); rb[:, 61:85] = knees.reshape(N, 24)
    rbp = rb.clone(); rbp[:, 0:36] += draws(22, (N, 36), lo=-0.05, hi=0.05)[0]; rbp[:, 36:39] += 0.01
    rbuf, abuf = rbp.clone(), ap.clone()
    return Case([(rbuf, rb, rbp), (abuf, a1, ap)], lambda: (e.task_eval(rbuf, abuf, *o), o)[1], lambda: internal(e), keep=[e])


# ------------------------------------------------------------------------------------------------ policy and records
def policy_block(kind, nobs=64):
    """(model, packed forward block, log_std) of a fixed-seed policy."""
    torch.manual_seed(11)
    if kind == "gnn":
        from locomanipulationrl_amd.policies.graph_model import GraphPolicy, pack_gnn_params
        m = GraphPolicy().to(DEV); packed = pack_gnn_params(m.net, m.mean_layer, m.value_layer)
    else:
        from locomanipulationrl_amd.policies.mlp_model import SharedMLP, pack_mlp_params
        m = SharedMLP(nobs).to(DEV); packed = pack_mlp_params(m)
    return m, packed.contiguous(), torch.full((12,), -0.5, device=DEV)


def forward_case(cid, kind, nobs, fn):
    @case(cid)
    def build(rm, mp):
        _, packed, _ = policy_block(kind, nobs)
        real, poison = draws(31, (N, nobs), (N, nobs), lo=-2.0, hi=2.0)
        buf = poison.clone()
        return Case([(buf, real, poison)], lambda: list(fn(buf, packed)))


def _mlp_forward_plain(obs, packed):
    """lm_mlp_forward, the 64-wide prototype without num_obs (the wrappers go through lm_mlp_forward_obs)."""
    from locomanipulationrl_amd.lib import load_library
    lib = load_library()
    mean, value = torch.empty(obs.shape[0], 12, device=DEV), torch.empty(obs.shape[0], 1, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.lm_mlp_forward(p(obs), obs.shape[0], p(packed), p(mean), p(value), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    return mean, value


def _mlp_obs(obs, packed):
    from locomanipulationrl_amd.policies.mlp_model import mlp_forward_hip
    return mlp_forward_hip(obs, packed)


def _gnn(obs, packed):
    from locomanipulationrl_amd.policies.graph_model import gnn_forward_hip
    return gnn_forward_hip(obs, packed)


forward_case("mlp_forward", "mlp", 64, _mlp_forward_plain)
forward_case("mlp_forward_obs_64", "mlp", 64, _mlp_obs)
forward_case("mlp_forward_obs_88", "mlp", 88, _mlp_obs)
forward_case("gnn_forward", "gnn", 64, _gnn)


@case("sample_actions")
def _sample_actions(rm, mp):
    """Reads the engine's counters: the producer is a step that advances them; the mean block is poisoned as well."""
    from locomanipulationrl_amd.lib import sample_actions
    e = engine(rm, mp, [loco_params()])
    o, a1, ap, _ = warmed(e)
    mean, mean_p = draws(32, (N, 12), (N, 12))
    abuf, mbuf = ap.clone(), mean_p.clone()
    log_std = torch.full((12,), -0.5, device=DEV)
    return Case([(abuf, a1, ap), (mbuf, mean, mean_p)], lambda: o + list(sample_actions(e, mbuf, log_std, 9)), lambda: internal(e),
                producer=lambda: e.step(abuf, None, *o), keep=[e])


def _episode(e, o):
    from locomanipulationrl_amd.lib import EpisodeRecord
    rec = EpisodeRecord(e)
    return (lambda: (rec.update(o[2], o[3]), [rec.record])[1]), []


def _trajectory(e, o):
    from locomanipulationrl_amd.lib import TrajectoryRecord
    rec = TrajectoryRecord(e, [0, 17, 39], max_rows=4, episode_cap=0)
    return (lambda: (rec.update(o[2], o[3]), [rec.rows, rec.header])[1]), []


def _replay(e, o):
    from locomanipulationrl_amd.lib import ReplayPlan, ReplayRecord
    rng = np.random.default_rng(5)
    recs = [np.cumsum(rng.uniform(-0.02, 0.02, (6, 12)), axis=0), np.cumsum(rng.uniform(-0.02, 0.02, (5, 12)), axis=0)]
    env_rec = np.arange(N, dtype=np.int32) % 3 - 1          # -1: takes no part
    plan = ReplayPlan(e, recs, env_rec, hold=1, window_rows=2)
    rec = ReplayRecord(e)
    nxt = torch.full((N, 12), 9.0, device=DEV)
    return (lambda: (rec.update(plan, 1, o[0], o[2], nxt), [rec.record, nxt])[1]), [plan]


def record_case(cid, make_call):
    """The record updates read what the step before them wrote (outputs, state, counters): the producer is that step."""
    @case(cid)
    def build(rm, mp):
        e = engine(rm, mp, [loco_params()])
        o, a1, ap, _ = warmed(e)
        buf = ap.clone()
        update, owned = make_call(e, o)
        return Case([(buf, a1, ap)], lambda: o + update(), lambda: internal(e), producer=lambda: e.step(buf, None, *o), keep=owned + [e])


record_case("episode_update", _episode)
record_case("trajectory_update", _trajectory)
record_case("replay_update", _replay)


# ------------------------------------------------------------------------------------------------ rollouts
def rollout_case(cid, kind, mode, records=False):
    @case(cid)
    def build(rm, mp):
        from locomanipulationrl_amd.lib import POLICY_GNN, POLICY_MLP, EpisodeRecord, Rollout, TrajectoryRecord
        e = engine(rm, mp, [loco_params()])
        o, _, _, _ = warmed(e)
        _, packed, log_std = policy_block(kind)
        kw, extra = {}, []
        if records:
            er, tr = EpisodeRecord(e), TrajectoryRecord(e, [0, 17, 39], max_rows=2 * T - 1, episode_cap=0)          # the last row is dropped, and counted
            kw = dict(episode_record=er, trajectory_record=tr); extra = [er.record, tr.rows, tr.header]
        ro = Rollout(e, POLICY_GNN if kind == "gnn" else POLICY_MLP, packed, log_std, T, noise_seed=7, **kw)
        real = o[0].clone()
        poison, real2 = draws(41, (N, 64), (N, 64))
        ro.obs[0].copy_(poison)
        torch.cuda.synchronize()
        buffers = [ro.obs, ro.actions, ro.logp, ro.values, ro.rewards, ro.dones, ro.extras] + extra

        def call():
            ro.run(mode)
            return buffers

        def again(S):
            """The instantiated graph once more, on a second stream ordered after S by an event, from a new obs[0]."""
            if S is None:
                ro.obs[0].copy_(real2); ro.run(mode)
                return [b.clone() for b in buffers]
            S2 = torch.cuda.Stream()
            if S2 == S: S2 = torch.cuda.Stream()
            S2.wait_event(S.record_event())
            with torch.cuda.stream(S2):
                ro.obs[0].copy_(real2); ro.run(mode)
                return [torch.empty_like(b).copy_(b) for b in buffers]
        return Case([(ro.obs[0], real, poison)], call, lambda: internal(e), after=again if mode == "graph" else None, keep=[ro, e])


for _k in ("mlp", "gnn"):
    for _m in ("enqueue", "graph", "persistent"):
        rollout_case(f"rollout_{_k}_{_m}", _k, _m)
rollout_case("rollout_records_graph", "mlp", "graph", records=True)


# ------------------------------------------------------------------------------------------------ training
@case("gae")
def _gae(rm, mp):
    from locomanipulationrl_amd.policies.mlp_model import gae
    real = draws(51, (T, N), (T, N), (N,)); poison = draws(52, (T, N), (T, N), (N,))
    dones, dones_p = [(d > 0.6).long() for d in draws(53, (T, N), (T, N))]
    real.append(dones); poison.append(dones_p)
    bufs = [p.clone() for p in poison]
    return Case(list(zip(bufs, real, poison)), lambda: list(gae(bufs[0], bufs[1], bufs[3], bufs[2], 0.99, 0.95)))


def grad_case(cid, kind, nobs):
    @case(cid)
    def build(rm, mp):
        m, _, _ = policy_block(kind, nobs)
        if kind == "gnn":
            from locomanipulationrl_amd.policies.graph_model import bind_gnn_flat_params as bind, gnn_ppo_grad as grad_fn, gnn_ppo_grad_workspace
            ws = gnn_ppo_grad_workspace(B, DEV)
        else:
            from locomanipulationrl_amd.policies.mlp_model import bind_flat_params as bind, mlp_ppo_grad as grad_fn, ppo_grad_workspace
            ws = ppo_grad_workspace(nobs, B, DEV)
        flat, _, _ = bind(m)

        def batch(seed):
            obs, act, lp, val, adv, ret = draws(seed, (B, nobs), (B, 12), (B,), (B,), (B,), (B,))
            return [obs, act, lp * 0.5 - 13.0, val, adv, ret]          # old log-probabilities near those of the policy: moderate ratios
        real, poison = batch(61), batch(62)
        bufs = [p.clone() for p in poison]
        grad, stats = torch.zeros_like(flat), torch.zeros(4, device=DEV)
        return Case(list(zip(bufs, real, poison)), lambda: list(grad_fn(flat, *bufs, grad=grad, stats=stats, workspace=ws)))


grad_case("mlp_ppo_grad_64", "mlp", 64)
grad_case("mlp_ppo_grad_88", "mlp", 88)
grad_case("gnn_ppo_grad", "gnn", 64)


@case("optim_state_init")
def _optim_state_init(rm, mp):
    """No device input: the producer writes junk into the block the call then initialises - a call that ran early would be overwritten."""
    from locomanipulationrl_amd.policies.optim import optim_state
    state = optim_state(DEV, 1.0, 0)
    poison, junk = torch.full_like(state, 7.0), torch.full_like(state, 9.0)
    state.copy_(poison)
    return Case([(state, junk, poison)], lambda: [optim_state(DEV, 1e-3, 4, state=state)])


@case("adam_clip_step")
def _adam(rm, mp):
    from locomanipulationrl_amd.policies.optim import adam_clip_step, optim_state
    n = 1003          # a scalar tail behind the 16-byte vectors
    p, g, m, v, pp, gp = draws(71, (n,), (n,), (n,), (n,), (n,), (n,))
    m = m * 0.1; v = v * v * 0.01
    state = optim_state(DEV, 3e-4, 2)
    pbuf, gbuf = pp.clone(), gp.clone()

    def call():
        adam_clip_step(pbuf, gbuf, m, v, state, max_norm=1.0, clamp=(5, 12, -0.5))
        return [pbuf, m, v, state]
    return Case([(gbuf, g * 3.0, gp), (pbuf, p, pp)], call)


@case("kl_adaptive_lr")
def _kl(rm, mp):
    from locomanipulationrl_amd.policies.optim import kl_adaptive_lr, optim_state
    state = optim_state(DEV, 3e-4, 2)
    real, poison = torch.tensor([0.05, 0.07], device=DEV), torch.tensor([0.001, 0.002], device=DEV)          # the rate falls / rises
    buf = poison.clone()
    return Case([(buf, real, poison)], lambda: (kl_adaptive_lr(state, buf, 0.012), [state])[1])


def pack_case(cid, kind):
    @case(cid)
    def build(rm, mp):
        from locomanipulationrl_amd.policies.prepare import pack_params, scaler_state
        m, packed0, _ = policy_block(kind)
        if kind == "gnn":
            from locomanipulationrl_amd.policies.graph_model import bind_gnn_flat_params as bind
        else:
            from locomanipulationrl_amd.policies.mlp_model import bind_flat_params as bind
        flat, _, _ = bind(m)
        real, poison = flat.clone(), flat * 0.5 + 0.01
        st = scaler_state(64, DEV); stp = st.clone()
        st[:64] = draws(81, (64,))[0].double(); st[64:128] = draws(82, (64,), lo=0.5, hi=2.0)[0].double()
        fbuf, sbuf = poison.clone(), stp.clone()
        packed, status = torch.full_like(packed0, -777.0), torch.zeros(1, device=DEV, dtype=torch.int32)
        return Case([(fbuf, real, poison), (sbuf, st, stp)], lambda: [pack_params(kind, fbuf, 64, packed, status, sbuf), status])


pack_case("mlp_pack_params", "mlp")
pack_case("gnn_pack_params", "gnn")


def _prep_batch(seed):
    obs, ret, val, adv = draws(seed, (B, 64), (B,), (B,), (B,), lo=-2.0, hi=2.0)
    return [obs, ret, val, adv]


@case("batch_stats")
def _batch_stats(rm, mp):
    from locomanipulationrl_amd.policies.prepare import batch_stats, batch_stats_workspace
    real, poison = _prep_batch(91), _prep_batch(92)
    bufs = [p.clone() for p in poison]
    sums, ws = torch.zeros(2 * 64 + 5, device=DEV, dtype=torch.float64), batch_stats_workspace(B, 64, DEV)
    return Case(list(zip(bufs, real, poison)), lambda: [batch_stats(bufs[0], bufs[1], bufs[3], sums, ws), ws[:1]])


@case("batch_apply")
def _batch_apply(rm, mp):
    from locomanipulationrl_amd.policies.prepare import batch_apply, batch_stats, scaler_state
    real, poison = _prep_batch(91), _prep_batch(92)
    real.append(batch_stats(real[0], real[1], real[3])); poison.append(batch_stats(poison[0], poison[1], poison[3]))
    bufs = [p.clone() for p in poison]
    obs_state, val_state = scaler_state(64, DEV), scaler_state(1, DEV)
    out = tuple(torch.zeros_like(t) for t in bufs[:4])
    torch.cuda.synchronize()

    def call():
        batch_apply(bufs[0], bufs[1], bufs[2], bufs[3], bufs[4], obs_state, val_state, out=out)
        return list(out) + [obs_state, val_state]
    return Case(list(zip(bufs, real, poison)), call)


@pytest.mark.parametrize("cid", list(CASES))
def test_on_a_callers_stream(cid, robot_model, monkeypatch, rig):
    want = run_baseline(CASES[cid](robot_model, monkeypatch))
    got, window = run_on_stream(CASES[cid](robot_model, monkeypatch), rig)
    assert window, WINDOW_CLOSED
    assert_same_bits(got, want, cid)


def test_control_the_poison_discriminates(robot_model, monkeypatch, rig):
    """The same delay and poison, but the step is enqueued on the DEFAULT stream while S is still delayed: it reads the poison, and its bits differ
    from the baseline's.  So a launch that left S in a case above would have been seen."""
    build = CASES["step_w1"]
    want = run_baseline(build(robot_model, monkeypatch))
    c = build(robot_model, monkeypatch)
    S = rig.S
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        rig.delay()
        for buf, real, _ in c.bufs:
            buf.copy_(real)
    out = [o.clone() for o in c.call()]          # the default stream
    probe = c.bufs[0][0].clone()
    S.synchronize(); torch.cuda.synchronize()
    assert torch.equal(bits(probe), bits(c.bufs[0][2])), WINDOW_CLOSED
    got = [bits(o) for o in out] + [bits(s) for s in c.state()]
    c.close()
    differ = [k for k, (x, y) in enumerate(zip(got, want)) if not torch.equal(x, y)]
    assert 0 in differ and 2 in differ, ("observations and rewards of a step on poisoned actions equal the baseline's", differ)


# ------------------------------------------------------------------------------------------------ one trainer iteration
def _trainer():
    import locomanipulationrl_amd as lm
    from locomanipulationrl_amd.policies.mlp_model import SharedMLP
    from locomanipulationrl_amd.train.ppo import PPO
    torch.manual_seed(5)
    env = lm.make_env("QuadrupedPoseControl", num_envs=16, seed=5)
    ppo = PPO(env, SharedMLP(64).to(DEV), hip_update=True, hip_optimizer=True, hip_prepare=True, rollouts=6, learning_epochs=2)
    obs = env.reset()["obs"]
    obs, last_value, _ = ppo.collect(obs)          # the warm-up iteration, on the default stream
    ppo.update(last_value, fetch=False)
    torch.cuda.synchronize()
    return env, ppo, obs.clone()


def _trainer_state(env, ppo):
    ro = ppo.rollout
    return [bits(t) for t in (ppo._flat, ppo._m, ppo._v, ppo._ostate, ppo.obs_scaler.state, ppo.val_scaler.state, ppo._packed, ro.obs, ro.actions, ro.logp,
                              ro.values, ro.rewards, ro.dones, ro.extras)] + [bits(s) for s in internal(env._task.engine)]


def test_trainer_iteration_on_a_callers_stream(rig):
    """PPO(hip_update, hip_optimizer, hip_prepare), 16 envs, T = 6, 2 epochs: after one warm-up iteration a whole collect() + update(fetch=False)
    under S behind the delay leaves the bits of the same iteration on the default stream in the parameters, Adam's moments, the optimiser state,
    both scaler blocks, the packed block, the rollout buffers and the engine."""
    env, ppo, obs = _trainer()
    obs, last_value, _ = ppo.collect(obs)
    ppo.update(last_value, fetch=False)
    torch.cuda.synchronize()
    want = _trainer_state(env, ppo)
    env.close()

    env, ppo, real = _trainer()
    poison = draws(95, tuple(real.shape))[0]
    buf = poison.clone()
    S = rig.S
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        rig.delay()
        buf.copy_(real)
        t0 = time.perf_counter()
        _, last_value, _ = ppo.collect(buf)
        ppo.update(last_value, fetch=False)
        enqueue_ms = 1e3 * (time.perf_counter() - t0)
    probe = buf.clone()
    S.synchronize(); torch.cuda.synchronize()
    print(f"[streams] trainer iteration: enqueued in {enqueue_ms:.2f} ms of host time; the delay is {DELAY_MS} ms")
    assert torch.equal(bits(probe), bits(poison)), WINDOW_CLOSED
    got = _trainer_state(env, ppo)
    env.close()
    assert_same_bits(got, want, "trainer iteration")


# ------------------------------------------------------------------------------------------------ setters against work in flight
def _setter_values(rm, row):
    geo = np.geomspace(0.5, 2.0, N)
    if row == "mu":
        p0 = np.linspace(0.2, 1.2, N)
    elif row == "body_masses":
        p0 = np.asarray([rm.mass[k] for k in rm.table_body_order()])[:, None] * geo[None, :]
    else:
        p0 = loco_params().kd * geo
    return p0.astype(np.float32), np.ascontiguousarray(p0[..., ::-1]).astype(np.float32)


@pytest.mark.parametrize("row", ["mu", "body_masses", "kd"])          # a physics row, a mass row, an actuator row
@pytest.mark.parametrize("setter", ["set", "clear"])
def test_setters_against_work_in_flight(setter, row, robot_model, monkeypatch, rig):
    """lm_set_env_params / lm_clear_env_params called from the host while a step is still queued on S behind the delay: when the call returns, every
    step enqueued before it has run with the old rows and every later step sees the new ones.  Equal to the default-stream sequence step(a1)
    under P0, the setter, step(a2).  The mass and the actuator row take the record read-modify-write path of lm_clear_env_params."""
    p0, p1 = _setter_values(robot_model, row)

    def build():
        e = engine(robot_model, monkeypatch, [loco_params(dr_enabled=1)]); e.enable_env_params()
        e.set_env_params(**{row: p0})
        o, a1, ap, a2 = warmed(e)
        return e, o, outs(N), a1, ap, a2

    def change(e):
        e.set_env_params(**{row: p1}) if setter == "set" else e.clear_env_params(row)

    def result(e, o1, o2):
        return [bits(x) for x in o1 + o2 + internal(e)]

    e, o1, o2, a1, _, a2 = build()
    e.step(a1, None, *o1); change(e); e.step(a2, None, *o2)
    torch.cuda.synchronize()
    want = result(e, o1, o2); e.close()

    e, o1, o2, a1, ap, a2 = build()
    buf = ap.clone()
    S = rig.S
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        rig.delay()
        buf.copy_(a1)
        e.step(buf, None, *o1)
        queued = S.record_event()
    in_flight = not queued.query()          # asked just before the setter: the step has not run yet
    change(e)
    with torch.cuda.stream(S):
        e.step(a2, None, *o2)
    S.synchronize(); torch.cuda.synchronize()
    got = result(e, o1, o2); e.close()
    assert in_flight, WINDOW_CLOSED
    assert_same_bits(got, want, f"{setter} {row}")


# ------------------------------------------------------------------------------------------------ caller-captured graphs
def _chain(e, packed, log_std, o, rec):
    """MLP forward -> sample_actions -> engine.step with all outputs -> EpisodeRecord.update; the step's observations feed the next forward."""
    from locomanipulationrl_amd.lib import sample_actions
    from locomanipulationrl_amd.policies.mlp_model import mlp_forward_hip
    mean, value = mlp_forward_hip(o[0], packed)
    act, logp = sample_actions(e, mean, log_std, 9)
    e.step(act, None, *o)
    rec.update(o[2], o[3])
    return [mean, value, act, logp]


def _graph_and_twin(rm, mp, make, between=None):
    """Engine A replays a torch.cuda.graph of one iteration five times, its twin B runs the five iterations eagerly; compared after each."""
    from locomanipulationrl_amd.lib import EpisodeRecord
    sides = []
    for _ in range(2):
        e = make(rm, mp)
        _, packed, log_std = policy_block("mlp")
        o = outs(N); rec = EpisodeRecord(e)
        e.step(draws(11, (N, 12))[0], None, *o)          # the warm-up: an eager step
        _chain(e, packed, log_std, o, rec)               # ... and an eager iteration (every lazy initialisation is behind us)
        torch.cuda.synchronize()
        sides.append((e, packed, log_std, o, rec))
    (ea, *a), (eb, *b) = sides
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):          # a linear, single-stream graph
        ra = _chain(ea, *a)
    for it in range(5):
        if between and it == 2:
            torch.cuda.synchronize()
            between(ea); between(eb)
        g.replay()
        rb = _chain(eb, *b)
        torch.cuda.synchronize()
        got = [bits(x) for x in ra + a[2] + [a[3].record] + internal(ea)]
        want = [bits(x) for x in rb + b[2] + [b[3].record] + internal(eb)]
        assert_same_bits(got, want, f"replay {it + 1}")
    moved = bool((a[3].record[1] > 0).any()) or bool((a[3].record[2] > 0).any())
    del g
    ea.close(); eb.close()
    assert moved, "the episode record never moved"


def test_caller_graph_replays_equal_eager(robot_model, monkeypatch):
    """A hipGraph the CALLER captured around lm_step (un-randomised engine): five replays equal five eager iterations of a twin."""
    _graph_and_twin(robot_model, monkeypatch, lambda rm, mp: engine(rm, mp, [loco_params()]))


def test_caller_graph_sees_new_env_params(robot_model, monkeypatch):
    """'Holding, changing or clearing rows afterwards needs no re-capture': set_env_params between replay 2 and replay 3 of a graph captured before it;
    replays 3 to 5 equal the eager twin that made the same change."""
    p1 = np.linspace(1.1, 0.3, N).astype(np.float32)
    _graph_and_twin(robot_model, monkeypatch, _env_params_engine, between=lambda e: e.set_env_params(mu=p1))
