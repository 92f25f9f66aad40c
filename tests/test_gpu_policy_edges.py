"""The stochastic policy path on the MI355X against references outside the library (tests/policy_reference.py, proven on the CPU by
tests/test_policy_reference_host.py; the torch modules in float64):
  (a) lm_sample_actions against the float64 reference on synthetic counter blocks, inside sentinel-filled buffers;
  (b) the fused sampling epilogues at N = 1 and N = 17: enqueue, graph and persistent rollouts bit-equal to a step-by-step run whose samples
      are checked against the reference with the counters read before each step;
  (c) the policy tiles at batches that do not fill a 16-sample tile: float64 accuracy by the project's yardstick (4 x torch fp32's error over the
      whole pool + 2e-7 x scale), bit-equality with the same rows of a whole-pool launch, guard floats around the outputs;
  (d) misaligned parameter / observation pointers are refused before anything is launched.
The C entry points are called through ctypes so that every output sits inside a larger sentinel-filled buffer.
Bounds: policy_reference.EPS_BOUND / action_bound / logp_bound (derived there).  Measured maxima: DESIGN.md 5.5."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import policy_reference as R

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, -777.0


def _lib():
    from locomanipulationrl_amd.lib import build_library, load_library
    build_library()
    return load_library()


def P(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def guarded(n):
    """(buffer, payload view of n floats with GUARD sentinel floats on each side)."""
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ (a) lm_sample_actions
def run_sampler(mean, log_std, cnt, seed):
    """lm_sample_actions into guarded buffers -> (actions [N][12], logp [N]) as float64 numpy, guards checked."""
    lib = _lib()
    N = mean.shape[0]
    abuf, act = guarded(N * 12); lbuf, logp = guarded(N)
    rc = lib.lm_sample_actions(P(mean), P(log_std), P(cnt), N, C.c_uint32(seed), P(act), P(logp), stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.lm_last_error()
    assert guards_intact(abuf, N * 12), "guard floats around actions were written"
    assert guards_intact(lbuf, N), "guard floats around logp were written"
    return act.clone().reshape(N, 12), logp.clone()


def check_samples(tag, act_dev, logp_dev, mean, log_std, cnt, seed):
    """Device samples (torch, fp32) against sample_ref with the bounds of policy_reference; prints and returns the worst error / bound."""
    mean64 = mean.double().cpu().numpy(); ls64 = log_std.double().cpu().numpy()
    eps, act, logp = R.sample_ref(mean64, ls64, cnt, seed)
    ea = np.abs(act_dev.double().cpu().numpy() - act) / R.action_bound(mean64, ls64, eps)
    el = np.abs(logp_dev.double().cpu().numpy() - logp) / R.logp_bound(ls64, eps)
    print(f"{tag}: action error / bound {ea.max():.3f}, logp error / bound {el.max():.3f}")
    assert np.isfinite(ea).all() and np.isfinite(el).all()
    assert ea.max() <= 1.0, (tag, "actions", float(ea.max()), np.unravel_index(ea.argmax(), ea.shape))
    assert el.max() <= 1.0, (tag, "logp", float(el.max()), int(el.argmax()))
    return float(ea.max()), float(el.max())


@pytest.mark.parametrize("seed", [0, 77, 0xFFFFFFFF])
@pytest.mark.parametrize("N", [1, 255, 257, 4099])
def test_sampler_matches_the_float64_reference_on_synthetic_counters(N, seed):
    rng = np.random.default_rng(1000 * N + (seed & 0xFFFF))
    cnt = R.synthetic_counters(N, rng)
    cnt_dev = torch.as_tensor(cnt, device="cuda")
    # mean = 0, log_std = 0: actions = fmaf(1, eps, 0) = eps exactly
    zero = torch.zeros(N, 12, device="cuda"); ls0 = torch.zeros(12, device="cuda")
    a0, lp0 = run_sampler(zero, ls0, cnt_dev, seed)
    eps_ref, _, _ = R.sample_ref(np.zeros((N, 12)), np.zeros(12), cnt, seed)
    err = np.abs(a0.double().cpu().numpy() - eps_ref)
    print(f"N {N} seed {seed:#x}: largest |eps_dev - eps_ref| {err.max():.3e} (bound {R.EPS_BOUND:g})")
    assert err.max() <= R.EPS_BOUND, np.unravel_index(err.argmax(), err.shape)
    check_samples(f"N {N} seed {seed:#x} unit", a0, lp0, zero, ls0, cnt, seed)
    # random means, log_std from {-20, -0.7, 0, 2} per action
    mean = torch.as_tensor(rng.standard_normal((N, 12)).astype(np.float32), device="cuda")
    ls = torch.as_tensor(rng.choice(np.array([-20.0, -0.7, 0.0, 2.0], dtype=np.float32), size=12), device="cuda")
    a1, lp1 = run_sampler(mean, ls, cnt_dev, seed)
    check_samples(f"N {N} seed {seed:#x} random", a1, lp1, mean, ls, cnt, seed)
    # two calls write the same bits
    a2, lp2 = run_sampler(mean, ls, cnt_dev, seed)
    assert torch.equal(a1, a2) and torch.equal(lp1, lp2)


# ------------------------------------------------------------------------------------------------ (b) fused epilogues at ragged sizes
def rollout_setup(policy):
    """(robot model, engine parameter blocks, split_env, num_obs, packed parameters, forward, policy kind)."""
    from locomanipulationrl_amd.engine_config import loco_params
    from locomanipulationrl_amd.lib import POLICY_GNN, POLICY_MLP
    from locomanipulationrl_amd.model.robot_model import load_model
    from locomanipulationrl_amd.policies.graph_model import GraphPolicy, gnn_forward_hip, pack_gnn_params
    from locomanipulationrl_amd.policies.mlp_model import SharedMLP, mlp_forward_hip, pack_mlp_params
    torch.manual_seed(3)
    if policy == "mlp88":
        from locomanipulationrl_amd.utils.config import SimConfig, load_config
        from locomanipulationrl_amd.utils.task_util import task_map
        name = "QuadrupedPoseControlCustomController"
        task = task_map()[name](name=name, sim_config=SimConfig(load_config(name, num_envs=32)), env=None)
        rm, params, split = load_model(task.model_asset), task.engine_params(), task.split_env()
    else:
        rm, params, split = load_model("quadruped_robot_v2"), [loco_params()], None
    nobs = params[0].num_obs
    if policy == "gnn":
        m = GraphPolicy().cuda(); packed = pack_gnn_params(m.net, m.mean_layer, m.value_layer).cuda(); return rm, params, split, nobs, packed, gnn_forward_hip, POLICY_GNN
    m = SharedMLP(num_observations=nobs).cuda()
    return rm, params, split, nobs, pack_mlp_params(m).cuda(), mlp_forward_hip, POLICY_MLP


@pytest.mark.parametrize("N", [1, 17])
@pytest.mark.parametrize("policy", ["mlp64", "mlp88", "gnn"])
def test_fused_sampling_at_ragged_sizes_equals_stepwise_and_the_reference(policy, N):
    from locomanipulationrl_amd.lib import Engine, Rollout, sample_actions
    T, noise_seed = 4, 77
    rm, params, split, nobs, packed, fwd, kind = rollout_setup(policy)
    assert nobs == (88 if policy == "mlp88" else 64)
    log_std = torch.linspace(-1.0, 0.2, 12, device="cuda")
    modes = ("enqueue", "graph", "persistent")          # un-randomised engines without contact reporting: the persistent kernel supports all three policies
    engines = [Engine(rm, params, N, split_env=split, seed=4) for _ in range(len(modes) + 1)]
    obs0 = []
    for e in engines:      # the reset step, to have observations to start from
        o = torch.empty(N, nobs, device="cuda"); e.step(torch.zeros(N, 12, device="cuda"), None, o); obs0.append(o)
    plans = []
    for e, o, mode in zip(engines, obs0, modes):
        r = Rollout(e, kind, packed, log_std, T, noise_seed=noise_seed); r.obs[0] = o; r.run(mode); plans.append(r)
    # step by step on the last engine: stand-alone forward, lm_sample_actions, lm_step; the counters read before each step key the reference
    e = engines[-1]; obs = obs0[-1]
    ref = dict(obs=[obs.clone()], act=[], logp=[], val=[], rew=[], done=[])
    worst = [0.0, 0.0]
    for t in range(T):
        mean, value = fwd(obs.contiguous(), packed)
        torch.cuda.synchronize()
        cnt = e.cnt.cpu().numpy().copy()
        act, logp = sample_actions(e, mean, log_std, noise_seed)
        w = check_samples(f"{policy} N {N} step {t}", act, logp, mean, log_std, cnt, noise_seed)
        worst = [max(a, b) for a, b in zip(worst, w)]
        o = torch.empty(N, nobs, device="cuda"); r = torch.empty(N, device="cuda"); d = torch.empty(N, dtype=torch.int64, device="cuda")
        e.step(act, None, o, None, r, d)
        ref["act"].append(act); ref["logp"].append(logp); ref["val"].append(value.reshape(-1)); ref["rew"].append(r); ref["done"].append(d); ref["obs"].append(o.clone())
        obs = o
    _, vlast = fwd(obs.contiguous(), packed); ref["val"].append(vlast.reshape(-1))
    torch.cuda.synchronize()
    for mode, ro, eng in zip(modes, plans, engines):
        for name, key in (("obs", "obs"), ("actions", "act"), ("logp", "logp"), ("values", "val"), ("rewards", "rew"), ("dones", "done")):
            a, b = getattr(ro, name), torch.stack(ref[key])
            assert torch.equal(a, b), (policy, N, mode, name, float((a.double() - b.double()).abs().max()))
        assert torch.equal(eng.state, e.state) and torch.equal(eng.cnt, e.cnt), (policy, N, mode)
    print(f"{policy} N {N}: worst action error / bound {worst[0]:.3f}, worst logp error / bound {worst[1]:.3f} over {T} steps")
    for r in plans: r.close()
    for eng in engines: eng.close()


# ------------------------------------------------------------------------------------------------ (c) policy tiles at small batches
POOL = 4096
SMALL = (1, 15, 16, 17, 33)
CASES = {"plain": (2.0, False), "scaler": (2.0, True), "tiny": (1e-4, False)}      # (factor on the pool, scaler folded in); tiny: the lo halves of the split go subnormal


def width(policy):
    return 88 if policy == "mlp88" else 64


@functools.lru_cache(maxsize=None)
def pool(nobs):
    """The seeded pool of 4096 unit-normal observations of that width (CPU, fp32); never modified."""
    return torch.randn(POOL, nobs, generator=torch.Generator().manual_seed(100 + nobs))


@functools.lru_cache(maxsize=None)
def tile_reference(policy, case):
    """CPU, computed once and shared: (obs fp32 [POOL][nobs], packed parameters, float64 mean [POOL][12] and value [POOL], e32 = torch fp32's largest
    error against float64 over the WHOLE pool)."""
    from locomanipulationrl_amd.policies.graph_model import GraphPolicy, pack_gnn_params
    from locomanipulationrl_amd.policies.mlp_model import SharedMLP, pack_mlp_params
    nobs = width(policy); factor, scaler = CASES[case]
    torch.manual_seed(11 + nobs + (policy == "gnn"))
    make = (lambda: GraphPolicy()) if policy == "gnn" else (lambda: SharedMLP(num_observations=nobs))
    m32 = make(); m64 = make().double(); m64.load_state_dict({k: v.double() for k, v in m32.state_dict().items()})
    obs = (pool(nobs) * factor).contiguous()
    mu = var = None
    if scaler:
        g = torch.Generator().manual_seed(7)
        mu = torch.randn(nobs, generator=g) * 0.3; var = torch.rand(nobs, generator=g) * 0.3 + 0.3
        xn = (obs.double() - mu.double()) / (var.double().sqrt() + 1e-8)
        hi, lo = float((xn > 5.0).double().mean()), float((xn < -5.0).double().mean())
        assert hi >= 0.01 and lo >= 0.01, (hi, lo)          # the clip is exercised on both sides
    def norm(x, dt):
        return x.to(dt) if mu is None else torch.clamp((x.to(dt) - mu.to(dt)) / (var.to(dt).sqrt() + 1e-8), -5.0, 5.0)
    with torch.no_grad():
        mr, _, vr = m64(norm(obs, torch.float64)); m_32, _, v_32 = m32(norm(obs, torch.float32))
    e32 = max(float((m_32.double() - mr).abs().max()), float((v_32.double() - vr).abs().max()))
    packed = pack_gnn_params(m32.net, m32.mean_layer, m32.value_layer, mu, var, 1e-8, 5.0) if policy == "gnn" else pack_mlp_params(m32, mu, var, 1e-8, 5.0)
    if case == "tiny":          # the premise of the case: the lo halves (x - fp16(x)) of the observations are fp16 subnormals
        lo_half = (obs - obs.half().float()).abs()
        assert float((lo_half < 2.0 ** -14).double().mean()) == 1.0 and float((lo_half > 0).double().mean()) > 0.9
    return obs, packed.contiguous(), mr, vr.reshape(-1), e32


def run_tile(policy, obs_dev, packed_dev):
    """The stand-alone forward through the C entry point into guarded buffers -> (mean [B][12], value [B]); guards checked."""
    lib = _lib()
    B = obs_dev.shape[0]
    mbuf, mean = guarded(B * 12); vbuf, value = guarded(B)
    if policy == "gnn": rc = lib.lm_gnn_forward(P(obs_dev), B, P(packed_dev), P(mean), P(value), stream())
    else: rc = lib.lm_mlp_forward_obs(P(obs_dev), B, obs_dev.shape[1], P(packed_dev), P(mean), P(value), stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.lm_last_error()
    assert guards_intact(mbuf, B * 12), (policy, B, "guard floats around mean were written")
    assert guards_intact(vbuf, B), (policy, B, "guard floats around value were written")
    return mean.clone().reshape(B, 12), value.clone()


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("policy", ["mlp64", "mlp88", "gnn"])
def test_policy_tiles_at_small_batches(policy, case):
    obs, packed, mr, vr, e32 = tile_reference(policy, case)
    obs_dev, packed_dev = obs.cuda(), packed.cuda()
    m_full, v_full = run_tile(policy, obs_dev, packed_dev)
    worst = 0.0
    for B in SMALL + (POOL,):
        if B == POOL: m, v = m_full, v_full
        else:
            m, v = run_tile(policy, obs_dev[:B].clone(), packed_dev)
            # a sample is one MFMA column: its arithmetic depends neither on the column nor on the block
            assert torch.equal(m, m_full[:B]) and torch.equal(v, v_full[:B]), (policy, case, B, float((m - m_full[:B]).abs().max()), float((v - v_full[:B]).abs().max()))
        err = max(float((m.double().cpu() - mr[:B]).abs().max()), float((v.double().cpu() - vr[:B]).abs().max()))
        scale = max(1.0, float(mr[:B].abs().max()), float(vr[:B].abs().max()))
        bound = 4.0 * e32 + 2e-7 * scale
        worst = max(worst, err / bound)
        assert bool(torch.isfinite(m).all()) and bool(torch.isfinite(v).all())
        assert err <= bound, (policy, case, B, err, e32, scale)
    print(f"{policy} {case}: torch fp32 error over the pool {e32:.3e}; worst tile err / (4 e32 + 2e-7 scale) {worst:.3f}")


# ------------------------------------------------------------------------------------------------ (d) argument hygiene
@pytest.mark.parametrize("policy", ["mlp64", "mlp88", "gnn"])
@pytest.mark.parametrize("which", ["params", "obs"])
def test_forward_refuses_a_misaligned_pointer(policy, which):
    """A pointer 4 bytes off a 16-byte boundary: -1 with a message, nothing launched (the sentinel-filled outputs come back untouched)."""
    lib = _lib()
    nobs = width(policy); B = 16
    n_par = lib.lm_gnn_param_count() if policy == "gnn" else lib.lm_mlp_param_count_obs(nobs)
    par = torch.zeros(n_par + 4, device="cuda"); obs = torch.zeros(B * nobs + 4, device="cuda")
    assert par.data_ptr() % 16 == 0 and obs.data_ptr() % 16 == 0
    off_p, off_o = (4, 0) if which == "params" else (0, 4)
    mbuf, mean = guarded(B * 12); vbuf, value = guarded(B)
    if policy == "gnn": rc = lib.lm_gnn_forward(P(obs, off_o), B, P(par, off_p), P(mean), P(value), stream())
    else: rc = lib.lm_mlp_forward_obs(P(obs, off_o), B, nobs, P(par, off_p), P(mean), P(value), stream())
    torch.cuda.synchronize()
    assert rc == -1 and b"16-byte aligned" in lib.lm_last_error()
    assert bool((mbuf == SENTINEL).all()) and bool((vbuf == SENTINEL).all())


@pytest.mark.parametrize("policy", ["mlp64", "gnn"])
@pytest.mark.parametrize("which", ["params", "obs"])
def test_rollout_create_refuses_a_misaligned_pointer(policy, which):
    from locomanipulationrl_amd.engine_config import loco_params
    from locomanipulationrl_amd.lib import Engine, POLICY_GNN, POLICY_MLP
    from locomanipulationrl_amd.model.robot_model import load_model
    lib = _lib()
    N, T = 16, 2
    eng = Engine(load_model("quadruped_robot_v2"), [loco_params()], N, seed=1)
    n_par = lib.lm_gnn_param_count() if policy == "gnn" else lib.lm_mlp_param_count_obs(64)
    par = torch.zeros(n_par + 4, device="cuda"); obs = torch.zeros((T + 1) * N * 64 + 4, device="cuda"); ls = torch.zeros(12, device="cuda")
    f = lambda *s: torch.full(s, SENTINEL, device="cuda")
    act, logp, val, rew, dones = f(T, N, 12), f(T, N), f(T + 1, N), f(T, N), torch.full((T, N), -7, dtype=torch.int64, device="cuda")
    off_p, off_o = (4, 0) if which == "params" else (0, 4)
    h = C.c_void_p()
    rc = lib.lm_rollout_create(C.byref(h), eng._h, POLICY_GNN if policy == "gnn" else POLICY_MLP, P(par, off_p), P(ls), T, C.c_uint32(1), P(obs, off_o),
                               P(act), P(logp), P(val), P(rew), P(dones), None)
    torch.cuda.synchronize()
    assert rc == -1 and not h.value and b"16-byte aligned" in lib.lm_last_error()
    assert all(bool((t == SENTINEL).all()) for t in (act, logp, val, rew)) and bool((dones == -7).all())
    # the aligned pointers are accepted
    rc = lib.lm_rollout_create(C.byref(h), eng._h, POLICY_GNN if policy == "gnn" else POLICY_MLP, P(par), P(ls), T, C.c_uint32(1), P(obs),
                               P(act), P(logp), P(val), P(rew), P(dones), None)
    assert rc == 0 and h.value
    lib.lm_rollout_destroy(h)
    eng.close()
