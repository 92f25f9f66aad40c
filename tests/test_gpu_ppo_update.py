"""The HIP PPO update on the MI355X (csrc/lm_ppo.hip): lm_mlp_ppo_grad against the float64 autograd gradient of train.ppo.ppo_loss with
torch's own fp32 autograd as the yardstick, its edge sizes, determinism, guard rows and argument checks; lm_gae bit for bit against
distributed.compute_gae; PPO(hip_update=True) against the torch update on one engine state, checkpoints across the two modes, and the
recipe's behaviour.

Accuracy criterion: per parameter tensor err = ||g - g64|| / ||g64||; e_t = the largest err of torch's fp32 autograd (CPU) over the whole
case list; the kernel passes at err <= 4 e_t (the factor the forward tiles are granted).  stats likewise per statistic.
Measured on the MI355X (kernel err / e_t, worst tensor per case): see DESIGN.md 5.4."""
import copy
import ctypes as C
import functools

import pytest
import torch

import ppo_grad_reference as R

pytestmark = pytest.mark.gpu

WIDTHS = (64, 88)
N_CASES = {64: 8, 88: 7}


def _lib():
    from locomanipulationrl_amd.lib import load_library
    return load_library()


@functools.lru_cache(maxsize=None)
def geometry(num_obs):
    """(tile, groups_max): a batch far beyond tile x compute units launches the largest grid."""
    from locomanipulationrl_amd.policies.mlp_model import ppo_grad_geometry
    return ppo_grad_geometry(num_obs, 1 << 24, "cuda:0")


@functools.lru_cache(maxsize=None)
def sizes(num_obs):
    tile, gmax = geometry(num_obs)
    return tuple(R.case_sizes(tile, gmax, num_obs))


@functools.lru_cache(maxsize=None)
def reference(B, num_obs):
    """(case, g64, s64, fp32 errors per tensor, fp32 errors per statistic): computed once on the CPU, shared, never modified."""
    c = R.case_for_size(B, num_obs)
    R.check_conditions(c)
    g64, s64 = R.autograd(c, torch.float64)
    g32, s32 = R.autograd(c, torch.float32)
    return c, g64, s64, R.tensor_errors(g32, g64, num_obs), R.stat_errors(s32, s64)


@functools.lru_cache(maxsize=None)
def yardstick():
    """e_t and the per-statistic yardsticks: torch fp32's largest error over the whole case list."""
    e_t, e_s = 0.0, [0.0] * 4
    for w in WIDTHS:
        for B in sizes(w):
            _, _, _, te, se = reference(B, w)
            e_t = max(e_t, max(te.values())); e_s = [max(a, b) for a, b in zip(e_s, se)]
    return e_t, e_s


def run_kernel(c, guard=False, ws_fill=None, ws=None):
    from locomanipulationrl_amd.policies.mlp_model import mlp_ppo_grad, ppo_grad_workspace
    dev = torch.device("cuda:0")
    params = R.flat_params(c.model).to(dev)
    d = lambda t: t.to(dev)
    P = params.numel()
    buf = torch.full((P + 128,), -777.0, device=dev); grad = buf[64:64 + P]
    if ws is None:
        n_ws = ppo_grad_workspace(c.num_obs, c.B, dev).numel()
        wbuf = torch.full((n_ws + 64,), -777.0, device=dev); ws = wbuf[:n_ws]
        if ws_fill is not None:
            ws.fill_(ws_fill)
    else:
        wbuf = None
    stats = torch.full((4,), -777.0, device=dev)
    mlp_ppo_grad(params, d(c.obs), d(c.act), d(c.old_logp), d(c.old_val), d(c.adv), d(c.ret), R.HYPER["rclip"], R.HYPER["vclip"], R.HYPER["vscale"],
                 R.HYPER["escale"], grad=grad, stats=stats, workspace=ws)
    torch.cuda.synchronize()
    if guard:
        assert bool((buf[:64] == -777.0).all()) and bool((buf[64 + P:] == -777.0).all()), "guard floats around grad were written"
        assert wbuf is None or bool((wbuf[ws.numel():] == -777.0).all()), "guard floats after the workspace were written"
    return grad.clone(), stats.clone(), ws


@pytest.mark.parametrize("num_obs,k", [(w, k) for w in WIDTHS for k in range(N_CASES[w])])
def test_gradient_and_stats_match_float64_within_fp32_yardstick(num_obs, k):
    B = sizes(num_obs)[k]
    c, g64, s64, te, se = reference(B, num_obs)
    e_t, e_s = yardstick()
    g, s, _ = run_kernel(c, guard=True, ws_fill=float("nan"))
    err = R.tensor_errors(g.cpu(), g64, num_obs); serr = R.stat_errors(s.cpu(), s64)
    print(f"num_obs {num_obs} B {B}: e_t {e_t:.3e}; kernel err / e_t worst {max(err.values()) / e_t:.3f} ({max(err, key=err.get)}); torch fp32 worst here {max(te.values()) / e_t:.3f}; "
          f"stats err / yardstick {[round(a / b, 3) for a, b in zip(serr, e_s)]}")
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(s).all())
    for name, e in err.items():
        assert e <= 4 * e_t, (name, e, e_t)
    for i, e in enumerate(serr):
        assert e <= 4 * e_s[i], (i, e, e_s[i])


def test_case_list_is_the_one_the_geometry_implies():
    for w in WIDTHS:
        tile, gmax = geometry(w)
        assert len(sizes(w)) == N_CASES[w] and tile >= 2 and gmax >= 1
        from locomanipulationrl_amd.policies.mlp_model import ppo_grad_geometry
        assert ppo_grad_geometry(w, gmax * tile, "cuda:0")[1] == gmax and ppo_grad_geometry(w, gmax * tile + 1, "cuda:0")[1] == gmax
        assert ppo_grad_geometry(w, tile + 1, "cuda:0")[1] == 2 and ppo_grad_geometry(w, 1, "cuda:0") == (tile, 1)


@pytest.mark.parametrize("num_obs", WIDTHS)
def test_single_sample_clipped_on_both_losses_gives_exact_zeros(num_obs):
    c = R.make_case(1, num_obs, seed=7, ratio_cls=[2], value_cls=[2], adv_sign=[1.0])      # ratio above the clip with a positive advantage; v - old_v above the clip
    k = R.check_conditions(c)
    assert not bool(k["pi_live"].any()) and not bool(k["v_live"].any())
    g, s, _ = run_kernel(c, guard=True, ws_fill=float("nan"))
    g = g.cpu()
    assert bool((g[:-12] == 0.0).all()), "a trunk / head / bias gradient is not exactly zero"
    assert bool((g[-12:] == -torch.tensor(R.HYPER["escale"], dtype=torch.float32)).all()), g[-12:]


@pytest.mark.parametrize("num_obs", WIDTHS)
def test_dead_and_masked_lanes_contribute_nothing(num_obs):
    B = 33
    i = torch.arange(B); odd = (i % 2) == 1
    ratio_cls = torch.where(odd, torch.zeros_like(i), i // 2 % 3)                 # odd: ratio below the clip ...
    sign = torch.where(odd, -torch.ones(B), 1.0 - 2.0 * ((i // 2) % 2).float())    # ... with a negative advantage: dead on the policy loss
    value_cls = torch.where(odd, torch.full_like(i, 2), (i // 6) % 3)             # odd: v - old_v above the clip: dead on the value loss
    c = R.make_case(B, num_obs, seed=11, ratio_cls=ratio_cls, value_cls=value_cls, adv_sign=sign)
    k = R.check_conditions(c, shares=False)
    assert not bool(k["pi_live"][odd].any()) and not bool(k["v_live"][odd].any()) and bool(k["pi_live"][~odd].any()) and bool(k["v_live"][~odd].any())
    live = copy.copy(c); live.B = int((~odd).sum())
    for name in ("obs", "act", "old_logp", "old_val", "adv", "ret"):
        setattr(live, name, getattr(c, name)[~odd].contiguous())
    g64_live, _ = R.autograd(live, torch.float64)
    share = live.B / B
    expect = g64_live * share
    expect[-12:] = (g64_live[-12:] + R.HYPER["escale"]) * share - R.HYPER["escale"]      # the entropy term is not a mean over samples
    g, _, _ = run_kernel(c, guard=True)
    e_t, _ = yardstick()
    err = R.tensor_errors(g.cpu(), expect, num_obs)
    print(f"num_obs {num_obs}: dead lanes, err / e_t worst {max(err.values()) / e_t:.3f}")
    for name, e in err.items():
        assert e <= 4 * e_t, (name, e, e_t)


@pytest.mark.parametrize("num_obs", WIDTHS)
@pytest.mark.parametrize("B", [40, 8197])
def test_two_calls_write_the_same_bits(num_obs, B):
    c = reference(B, num_obs)[0]
    g1, s1, ws = run_kernel(c, guard=True, ws_fill=float("nan"))
    g2, s2, _ = run_kernel(c, ws=ws)                       # on what the first call left in the workspace
    g3, s3, _ = run_kernel(c, ws_fill=12345.0)
    for a, b in ((g1, g2), (g1, g3), (s1, s2), (s1, s3)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_bad_arguments_are_refused_not_run():
    from locomanipulationrl_amd.lib import LmPpoHyper
    from locomanipulationrl_amd.policies.mlp_model import ppo_grad_workspace
    lib = _lib(); dev = torch.device("cuda:0")
    c = reference(40, 64)[0]
    params = R.flat_params(c.model).to(dev); P = params.numel()
    t = {n: getattr(c, n).to(dev) for n in ("obs", "act", "old_logp", "old_val", "adv", "ret")}
    grad = torch.full((P,), -777.0, device=dev); stats = torch.full((4,), -777.0, device=dev)
    ws = ppo_grad_workspace(64, 40, dev)
    hp = LmPpoHyper(0.2, 0.2, 1.0, 0.01)
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(params=params, obs=t["obs"], act=t["act"], olp=t["old_logp"], ov=t["old_val"], adv=t["adv"], ret=t["ret"], B=40, nobs=64, hp=hp, grad=grad, stats=stats, ws=ws, nbytes=None):
        nbytes = (ws.numel() * 4 if ws is not None else 0) if nbytes is None else nbytes
        return lib.lm_mlp_ppo_grad(p(params), p(obs), p(act), p(olp), p(ov), p(adv), p(ret), B, nobs, C.byref(hp) if hp is not None else None, p(grad), p(stats), p(ws), nbytes, s)

    with torch.cuda.device(dev):
        assert call() == 0
        for kw in (dict(params=None), dict(obs=None), dict(act=None), dict(olp=None), dict(ov=None), dict(adv=None), dict(ret=None), dict(hp=None), dict(grad=None),
                   dict(stats=None), dict(ws=None), dict(B=0), dict(B=-3), dict(nobs=70), dict(nobs=0)):
            assert call(**kw) == -1, kw
        grad.fill_(-777.0); torch.cuda.synchronize()
        assert call(nbytes=ws.numel() * 4 - 4) == -1 and b"workspace" in lib.lm_last_error()      # a short workspace is refused, never overrun
        assert call(B=8197) == -1                                                                # ... as is one sized for a smaller batch
        torch.cuda.synchronize()
        assert bool((grad == -777.0).all())
        assert call(params=R.flat_params(c.model)) == -1                                         # host memory is no buffer of the current device
        assert lib.lm_mlp_ppo_grad_workspace(70, 40) < 0 and lib.lm_mlp_ppo_grad_workspace(64, 0) < 0
        tile, groups = C.c_int(0), C.c_int(0)
        assert lib.lm_mlp_ppo_grad_geometry(64, 40, None, C.byref(groups)) == -1 and lib.lm_mlp_ppo_grad_geometry(70, 40, C.byref(tile), C.byref(groups)) == -1
        z = torch.zeros(4, device=dev); zi = torch.zeros(4, device=dev, dtype=torch.int64)
        assert lib.lm_gae(p(z), p(z), p(zi), p(z), 1, 4, 0.99, 0.95, p(z.clone()), p(z.clone()), s) == 0
        assert lib.lm_gae(None, p(z), p(zi), p(z), 1, 4, 0.99, 0.95, p(z), p(z), s) == -1 and lib.lm_gae(p(z), p(z), p(zi), p(z), 0, 4, 0.99, 0.95, p(z), p(z), s) == -1
    if torch.cuda.device_count() > 1:
        with torch.cuda.device(1):
            assert call() == -1 and b"current device" in lib.lm_last_error()


@pytest.mark.parametrize("T,N", [(1, 1), (5, 37), (48, 64), (48, 4099)])
@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (1.0, 0.0)])
def test_gae_equals_compute_gae_bit_for_bit(T, N, gamma, lam):
    from locomanipulationrl_amd.distributed import compute_gae
    from locomanipulationrl_amd.policies.mlp_model import gae
    g = torch.Generator().manual_seed(T * 10007 + N)
    rew = torch.randn(T, N, generator=g); val = 3.0 * torch.randn(T, N, generator=g); last = 3.0 * torch.randn(N, generator=g)
    dones = (torch.rand(T, N, generator=g) < 0.1).long()
    dones[0, 0] = 1; dones[T - 1, 0] = 1                    # dones at t = 0 and at t = T-1
    if N > 2:
        dones[:, 1] = 1; dones[:, 2] = 0                    # on every step of one env, on none of another
    ret_c, adv_c = compute_gae(rew, val, dones.float(), last, gamma, lam)
    d = lambda x: x.to("cuda:0")
    ret_t, adv_t = compute_gae(d(rew), d(val), d(dones).float(), d(last), gamma, lam)
    ret_k, adv_k = gae(d(rew), d(val), d(dones), d(last), gamma, lam)
    bits = lambda x: x.cpu().view(torch.int32)
    assert torch.equal(bits(ret_k), bits(ret_t)) and torch.equal(bits(adv_k), bits(adv_t))
    assert torch.equal(bits(ret_k), bits(ret_c)) and torch.equal(bits(adv_k), bits(adv_c))


# ------------------------------------------------------------------------------------------------ trainer
class _Stop(Exception):
    pass


def _trainer(hip_update, seed=5, T=6, n=64, **kw):
    import locomanipulationrl_amd as lm
    from locomanipulationrl_amd.policies.mlp_model import SharedMLP
    from locomanipulationrl_amd.train.ppo import PPO
    torch.manual_seed(seed)
    env = lm.make_env("QuadrupedPoseControl", num_envs=n, seed=seed)
    model = SharedMLP(64).to("cuda:0")
    return env, PPO(env, model, rollouts=T, hip_update=hip_update, **kw)


def test_trainer_first_minibatch_gradient_matches_the_torch_update():
    grads, batches, models = {}, {}, {}
    for mode in (False, True):
        env, ppo = _trainer(mode, grad_norm_clip=1e9, entropy_loss_scale=0.01)      # a clip that never binds: clip_grad_norm_ multiplies by 1.0
        obs = env.reset()["obs"]
        obs, last_value, _ = ppo.collect(obs)
        models[mode] = copy.deepcopy(ppo.model).double().cpu()

        def stop():
            raise _Stop
        ppo.opt.step = stop                                                           # the first mini-batch's gradient, before the optimiser sees it
        with pytest.raises(_Stop):
            ppo.update(last_value)
        named = dict(ppo.model.named_parameters())
        grads[mode] = torch.cat([named[k].grad.reshape(-1) for k in R.FLAT_ORDER]).detach().cpu()
        batches[mode] = {k: v.detach().cpu() for k, v in ppo.last_batch.items()}
        if mode:
            assert grads[mode].data_ptr() != 0 and all(named[k].grad.data_ptr() == ppo._gflat.data_ptr() + 4 * ppo._offsets[k][0] for k in R.FLAT_ORDER)
        env.close()
    bits = lambda x: x.contiguous().view(torch.int32)
    for k in ("ret", "adv", "obs_n", "act", "old_logp", "old_val_n", "ret_n"):       # lm_gae == compute_gae on a real rollout, bit for bit (adv: after the same normalisation)
        assert torch.equal(bits(batches[True][k]), bits(batches[False][k])), k
    b = {k: v.double() for k, v in batches[False].items()}
    m = models[False]
    from locomanipulationrl_amd.train.ppo import ppo_loss
    ppo_loss(m(b["obs_n"]), b["act"], b["old_logp"], b["old_val_n"], b["adv"], b["ret_n"], 0.2, 0.2, 1.0, 0.01)[0].backward()
    named = dict(m.named_parameters())
    g64 = torch.cat([(named[k].grad if named[k].grad is not None else torch.zeros_like(named[k])).reshape(-1) for k in R.FLAT_ORDER]).cpu()
    e_t, _ = yardstick()
    for mode in (False, True):
        err = R.tensor_errors(grads[mode], g64, 64)
        print(f"trainer, hip_update {mode}: err / e_t {({k: round(v / e_t, 3) for k, v in err.items()})}")
        for name, e in err.items():
            assert e <= 4 * e_t, (mode, name, e, e_t)


def test_checkpoints_load_across_the_two_update_modes(tmp_path):
    state = {}
    for mode in (False, True):
        env, ppo = _trainer(mode, learning_epochs=2)
        obs = env.reset()["obs"]
        obs, last_value, _ = ppo.collect(obs)
        st = ppo.update(last_value)
        assert all(v == v for v in st.values())
        ppo.save(str(tmp_path / f"ck_{int(mode)}.pt"))
        state[mode] = ppo.state_dict()
        env.close()
    for src in (False, True):
        env, ppo = _trainer(not src)
        ppo.load(str(tmp_path / f"ck_{int(src)}.pt"))
        got, want = ppo.state_dict(), state[src]
        for k in want["model"]:
            assert torch.equal(got["model"][k].view(torch.int32), want["model"][k].view(torch.int32)), k
        for sc in ("obs_scaler", "val_scaler"):
            for k in ("mean", "var", "count"):
                assert torch.equal(got[sc][k], want[sc][k]), (sc, k)
        assert got["lr"] == want["lr"]
        for i, s in want["optimizer"]["state"].items():
            for k, v in s.items():
                g = got["optimizer"]["state"][i][k]
                assert torch.equal(torch.as_tensor(g).cpu(), torch.as_tensor(v).cpu()), (i, k)
        if not src:      # a torch checkpoint in a hip_update trainer: the parameters are still views into the flat block the kernel reads
            named = dict(ppo.model.named_parameters())
            assert all(named[k].data_ptr() == ppo._flat.data_ptr() + 4 * ppo._offsets[k][0] for k in R.FLAT_ORDER)
            obs = env.reset()["obs"]; obs, last_value, _ = ppo.collect(obs); st = ppo.update(last_value)
            assert all(v == v for v in st.values())
        env.close()


def test_permuted_mini_batches_go_through_the_kernel():
    env, ppo = _trainer(True, mini_batches=2, learning_epochs=2)
    before = ppo._flat.clone()
    obs = env.reset()["obs"]; obs, last_value, _ = ppo.collect(obs)
    st = ppo.update(last_value)                      # 2 x 2 gathered mini-batches of 192 rows
    assert all(v == v for v in st.values()) and bool(torch.isfinite(ppo._flat).all()) and not torch.equal(before, ppo._flat)
    assert list(ppo._ws) == [192]
    env.close()


def test_hip_update_requires_the_mlp():
    import locomanipulationrl_amd as lm
    from locomanipulationrl_amd.policies.graph_model import GraphPolicy
    from locomanipulationrl_amd.train.ppo import PPO
    env = lm.make_env("QuadrupedPoseControl", num_envs=64, seed=1)
    with pytest.raises(ValueError, match="SharedMLP"):
        PPO(env, GraphPolicy().to("cuda:0"), hip_update=True)
    env.close()


def test_recipe_learns_with_the_hip_update():
    """QuadrupedPoseControl, 4096 envs, 9600 timesteps, seed 1: the bar of the project's seed sweeps."""
    env, ppo = _trainer(True, seed=1, T=48, n=4096)
    hist = ppo.train(9600, log_every=50, log=lambda r: None)
    print("hip_update run:", {k: hist[-1][k] for k in ("success_rate", "wall_s", "kl", "lr", "std")})
    env.close()
    assert hist[-1]["success_rate"] >= 0.95, hist[-1]
