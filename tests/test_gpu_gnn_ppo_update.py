"""The HIP PPO update of the GNN policy on the MI355X (csrc/lm_gnn_ppo.hip): lm_gnn_ppo_grad against the float64 autograd gradient of
train.ppo.ppo_loss through GraphPolicy with torch's own fp32 autograd as the yardstick, its edge sizes, the even split of an aggregation tie,
dead and masked lanes, determinism, guard floats and argument checks; PPO(gnn_hip_update=True) against the torch update on one engine state,
checkpoints across the two modes, permuted mini-batches and ten updates.

Accuracy criterion (the one of test_gpu_ppo_update.py): per parameter tensor err = ||g - g64|| / ||g64||; e_t = the largest err of torch's fp32
autograd (CPU) over the whole case list; the kernel passes at err <= 4 e_t.  stats likewise per statistic.  A zero reference tensor demands
exact zeros.  Measured on the MI355X (kernel err / e_t, worst tensor per case): see DESIGN.md 5.4."""
import copy
import ctypes as C
import functools

import pytest
import torch

import gnn_grad_reference as R

pytestmark = pytest.mark.gpu

N_CASES = 8
HY = R.HYPER


def _lib():
    from locomanipulationrl_amd.lib import load_library
    return load_library()


@functools.lru_cache(maxsize=None)
def geometry():
    """(tile, groups_max): a batch far beyond tile x compute units launches the largest grid."""
    from locomanipulationrl_amd.policies.graph_model import gnn_ppo_grad_geometry
    return gnn_ppo_grad_geometry(1 << 24, "cuda:0")


@functools.lru_cache(maxsize=None)
def sizes():
    return tuple(R.case_sizes(*geometry()))


@functools.lru_cache(maxsize=None)
def reference(B):
    """(case, g64, s64, fp32 errors per tensor, fp32 errors per statistic): computed once on the CPU, shared, never modified."""
    c = R.case_for_size(B)
    R.check_conditions(c)
    g64, s64 = R.autograd(c, torch.float64)
    g32, s32 = R.autograd(c, torch.float32)
    return c, g64, s64, R.tensor_errors(g32, g64), R.stat_errors(s32, s64)


@functools.lru_cache(maxsize=None)
def yardstick():
    """e_t and the per-statistic yardsticks: torch fp32's largest error over the whole case list (from the reference alone)."""
    e_t, e_s = 0.0, [0.0] * 4
    for B in sizes():
        _, _, _, te, se = reference(B)
        e_t = max(e_t, max(te.values())); e_s = [max(a, b) for a, b in zip(e_s, se)]
    return e_t, e_s


def run_kernel(c, guard=False, ws_fill=None, ws=None):
    from locomanipulationrl_amd.policies.graph_model import gnn_ppo_grad, gnn_ppo_grad_workspace
    dev = torch.device("cuda:0")
    params = R.flat_params(c.model).to(dev)
    d = lambda t: t.to(dev)
    P = params.numel()
    buf = torch.full((P + 128,), -777.0, device=dev); grad = buf[64:64 + P]
    sbuf = torch.full((4 + 128,), -777.0, device=dev); stats = sbuf[64:68]
    if ws is None:
        n_ws = gnn_ppo_grad_workspace(c.B, dev).numel()
        wbuf = torch.full((n_ws + 64,), -777.0, device=dev); ws = wbuf[:n_ws]
        if ws_fill is not None:
            ws.fill_(ws_fill)
    else:
        wbuf = None
    gnn_ppo_grad(params, d(c.obs), d(c.act), d(c.old_logp), d(c.old_val), d(c.adv), d(c.ret), HY["rclip"], HY["vclip"], HY["vscale"], HY["escale"],
                 grad=grad, stats=stats, workspace=ws)
    torch.cuda.synchronize()
    if guard:
        assert bool((buf[:64] == -777.0).all()) and bool((buf[64 + P:] == -777.0).all()), "guard floats around grad were written"
        assert bool((sbuf[:64] == -777.0).all()) and bool((sbuf[68:] == -777.0).all()), "guard floats around stats were written"
        assert wbuf is None or bool((wbuf[ws.numel():] == -777.0).all()), "guard floats after the workspace were written"
    return grad.clone(), stats.clone(), ws


@pytest.mark.parametrize("k", range(N_CASES))
def test_gradient_and_stats_match_float64_within_fp32_yardstick(k):
    B = sizes()[k]
    c, g64, s64, te, se = reference(B)
    e_t, e_s = yardstick()
    g, s, _ = run_kernel(c, guard=True, ws_fill=float("nan"))
    err = R.tensor_errors(g.cpu(), g64); serr = R.stat_errors(s.cpu(), s64)
    print(f"B {B}: e_t {e_t:.3e}; kernel err / e_t worst {max(err.values()) / e_t:.3f} ({max(err, key=err.get)}); torch fp32 worst here {max(te.values()) / e_t:.3f}; "
          f"stats err / yardstick {[round(a / b, 3) for a, b in zip(serr, e_s)]}")
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(s).all())
    for name, e in err.items():
        assert e <= 4 * e_t, (name, e, e_t)
    for i, e in enumerate(serr):
        assert e <= 4 * e_s[i], (i, e, e_s[i])


def test_case_list_is_the_one_the_geometry_implies():
    from locomanipulationrl_amd.policies.graph_model import gnn_ppo_grad_geometry
    tile, gmax = geometry()
    assert len(sizes()) == N_CASES and tile >= 2 and gmax >= 1
    assert gnn_ppo_grad_geometry(gmax * tile, "cuda:0")[1] == gmax and gnn_ppo_grad_geometry(gmax * tile + 1, "cuda:0")[1] == gmax
    assert gnn_ppo_grad_geometry(tile + 1, "cuda:0")[1] == 2 and gnn_ppo_grad_geometry(1, "cuda:0") == (tile, 1)


def test_aggregation_tie_splits_the_gradient_evenly():
    """graph_layer3.linear2.weight = 0: every message into a node of the last layer is elu(b2) exactly, in fp32 too, so every max of that layer
    is a tie among all incoming edges, and every sample is value-dead (nothing goes through the value head's max, whose tie rule is not
    pinned).  float64 autograd (amax) splits the gradient evenly among the tied edges; the gradient of graph_layer3.linear2.weight must match
    it within the bound of the accuracy test.  A kernel that routed the whole gradient to the first maximal edge fails here: the first-edge
    restatement of the reference, on the CPU, is off by tens of per cent on that tensor - so this test discriminates."""
    c = R.tie_case()
    k = R.check_conditions(c, shares=False, gap=None)
    assert c.B == 33 and not bool(k["v_live"].any())
    g64, s64 = R.autograd(c, torch.float64)
    name = "net.graph_layer3.linear2.weight"
    g_first, _ = R.autograd(c, torch.float64, forward=lambda m, o: R.restated_outputs(m, o, first_edge=True))
    e_t, e_s = yardstick()
    first = R.tensor_errors(g_first, g64)[name]
    assert first > 0.1 and first > 100 * 4 * e_t, (first, e_t)       # first-edge-wins is nowhere near the bound
    g, s, _ = run_kernel(c, guard=True, ws_fill=float("nan"))
    err = R.tensor_errors(g.cpu(), g64)
    print(f"tie case: {name} err / e_t {err[name] / e_t:.3f} (first-edge routing: {first / e_t:.1f}); worst tensor err / e_t {max(err.values()) / e_t:.3f}")
    for n, e in err.items():                                         # the tensors below the zeroed weight have a zero reference: exact zeros
        assert e <= 4 * e_t, (n, e, e_t)


def test_single_sample_clipped_on_both_losses_gives_exact_zeros():
    c = R.make_case(1, seed=7, ratio_cls=[2], value_cls=[2], adv_sign=[1.0])      # ratio above the clip with a positive advantage; v - old_v above the clip
    k = R.check_conditions(c)
    assert not bool(k["pi_live"].any()) and not bool(k["v_live"].any())
    g, s, _ = run_kernel(c, guard=True, ws_fill=float("nan"))
    g = g.cpu()
    assert bool((g[:-12] == 0.0).all()), "a layer / head / bias gradient is not exactly zero"
    assert bool((g[-12:] == -torch.tensor(HY["escale"], dtype=torch.float32)).all()), g[-12:]


def test_dead_and_masked_lanes_contribute_nothing():
    tile, _ = geometry()
    B = 2 * tile + 1
    i = torch.arange(B); odd = (i % 2) == 1
    ratio_cls = torch.where(odd, torch.zeros_like(i), i // 2 % 3)                 # odd: ratio below the clip ...
    sign = torch.where(odd, -torch.ones(B), 1.0 - 2.0 * ((i // 2) % 2).float())    # ... with a negative advantage: dead on the policy loss
    value_cls = torch.where(odd, torch.full_like(i, 2), (i // 6) % 3)             # odd: v - old_v above the clip: dead on the value loss
    c = R.make_case(B, seed=11, ratio_cls=ratio_cls, value_cls=value_cls, adv_sign=sign)
    k = R.check_conditions(c, shares=False)
    assert not bool(k["pi_live"][odd].any()) and not bool(k["v_live"][odd].any()) and bool(k["pi_live"][~odd].any()) and bool(k["v_live"][~odd].any())
    live = copy.copy(c); live.B = int((~odd).sum())
    for name in ("obs", "act", "old_logp", "old_val", "adv", "ret"):
        setattr(live, name, getattr(c, name)[~odd].contiguous())
    g64_live, _ = R.autograd(live, torch.float64)
    share = live.B / B
    expect = g64_live * share
    expect[-12:] = (g64_live[-12:] + HY["escale"]) * share - HY["escale"]      # the entropy term is not a mean over samples
    g, _, _ = run_kernel(c, guard=True)
    e_t, _ = yardstick()
    err = R.tensor_errors(g.cpu(), expect)
    print(f"dead lanes, B {B}: err / e_t worst {max(err.values()) / e_t:.3f}")
    for name, e in err.items():
        assert e <= 4 * e_t, (name, e, e_t)


@pytest.mark.parametrize("B", [40, 8197])
def test_two_calls_write_the_same_bits(B):
    c = reference(B)[0]
    g1, s1, ws = run_kernel(c, guard=True, ws_fill=float("nan"))
    g2, s2, _ = run_kernel(c, ws=ws)                       # on what the first call left in the workspace
    g3, s3, _ = run_kernel(c, ws_fill=12345.0)
    for a, b in ((g1, g2), (g1, g3), (s1, s2), (s1, s3)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_bad_arguments_are_refused_not_run():
    from locomanipulationrl_amd.lib import LmPpoHyper
    from locomanipulationrl_amd.policies.graph_model import gnn_ppo_grad_workspace
    lib = _lib(); dev = torch.device("cuda:0")
    c = reference(40)[0]
    params = R.flat_params(c.model).to(dev); P = params.numel()
    t = {n: getattr(c, n).to(dev) for n in ("obs", "act", "old_logp", "old_val", "adv", "ret")}
    grad = torch.full((P,), -777.0, device=dev); stats = torch.full((4,), -777.0, device=dev)
    ws = gnn_ppo_grad_workspace(40, dev)
    hp = LmPpoHyper(0.2, 0.2, 1.0, 0.01)
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(params=params, obs=t["obs"], act=t["act"], olp=t["old_logp"], ov=t["old_val"], adv=t["adv"], ret=t["ret"], B=40, hp=hp, grad=grad, stats=stats, ws=ws, nbytes=None):
        nbytes = (ws.numel() * 4 if ws is not None else 0) if nbytes is None else nbytes
        return lib.lm_gnn_ppo_grad(p(params), p(obs), p(act), p(olp), p(ov), p(adv), p(ret), B, C.byref(hp) if hp is not None else None, p(grad), p(stats), p(ws), nbytes, s)

    with torch.cuda.device(dev):
        assert call() == 0
        for kw in (dict(params=None), dict(obs=None), dict(act=None), dict(olp=None), dict(ov=None), dict(adv=None), dict(ret=None), dict(hp=None), dict(grad=None),
                   dict(stats=None), dict(ws=None), dict(B=0), dict(B=-3)):
            assert call(**kw) == -1, kw
        mis = torch.zeros(P + 4, device=dev)[1:1 + P].copy_(params)                               # 4 bytes off a 16-byte boundary
        assert call(params=mis) == -1 and b"aligned" in lib.lm_last_error()
        grad.fill_(-777.0); stats.fill_(-777.0); torch.cuda.synchronize()
        assert call(nbytes=ws.numel() * 4 - 4) == -1 and b"workspace" in lib.lm_last_error()      # a short workspace is refused, never overrun
        assert call(B=8197) == -1                                                                # ... as is one sized for a smaller batch
        torch.cuda.synchronize()
        assert bool((grad == -777.0).all()) and bool((stats == -777.0).all())
        assert call(params=R.flat_params(c.model)) == -1                                         # host memory is no buffer of the current device
        assert lib.lm_gnn_ppo_grad_workspace(0) < 0
        tile, groups = C.c_int(0), C.c_int(0)
        assert lib.lm_gnn_ppo_grad_geometry(40, None, C.byref(groups)) == -1 and lib.lm_gnn_ppo_grad_geometry(0, C.byref(tile), C.byref(groups)) == -1
    if torch.cuda.device_count() > 1:
        with torch.cuda.device(1):
            assert call() == -1 and b"current device" in lib.lm_last_error()


# ------------------------------------------------------------------------------------------------ trainer
class _Stop(Exception):
    pass


def _trainer(gnn_hip_update, seed=5, T=6, n=64, **kw):
    import locomanipulationrl_amd as lm
    from locomanipulationrl_amd.policies.graph_model import GraphPolicy
    from locomanipulationrl_amd.train.ppo import PPO
    torch.manual_seed(seed)
    env = lm.make_env("QuadrupedPoseControlVertical", num_envs=n, seed=seed)
    model = GraphPolicy().to("cuda:0")
    return env, PPO(env, model, rollouts=T, gnn_hip_update=gnn_hip_update, **kw)


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
        grads[mode] = torch.cat([named[k].grad.reshape(-1) for k in R.GNN_FLAT_ORDER]).detach().cpu()
        batches[mode] = {k: v.detach().cpu() for k, v in ppo.last_batch.items()}
        if mode:
            assert all(named[k].grad.data_ptr() == ppo._gflat.data_ptr() + 4 * ppo._offsets[k][0] for k in R.GNN_FLAT_ORDER)
        env.close()
    bits = lambda x: x.contiguous().view(torch.int32)
    for k in ("ret", "adv", "obs_n", "act", "old_logp", "old_val_n", "ret_n"):       # lm_gae == compute_gae on a real rollout, bit for bit (adv: after the same normalisation)
        assert torch.equal(bits(batches[True][k]), bits(batches[False][k])), k
    b = {k: v.double() for k, v in batches[False].items()}
    m = models[False]
    from locomanipulationrl_amd.train.ppo import ppo_loss
    ppo_loss(m(b["obs_n"]), b["act"], b["old_logp"], b["old_val_n"], b["adv"], b["ret_n"], 0.2, 0.2, 1.0, 0.01)[0].backward()
    named = dict(m.named_parameters())
    g64 = torch.cat([(named[k].grad if named[k].grad is not None else torch.zeros_like(named[k])).reshape(-1) for k in R.GNN_FLAT_ORDER]).cpu()
    e_t, _ = yardstick()
    for mode in (False, True):
        err = R.tensor_errors(grads[mode], g64)
        print(f"trainer, gnn_hip_update {mode}: err / e_t worst {max(err.values()) / e_t:.3f} ({max(err, key=err.get)})")
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
        assert set(got["model"]) == set(want["model"]) and got["model_class"] == want["model_class"] == "GraphPolicy"
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
        if not src:      # a torch checkpoint in a gnn_hip_update trainer: the parameters are still views into the flat block the kernel reads
            named = dict(ppo.model.named_parameters())
            assert all(named[k].data_ptr() == ppo._flat.data_ptr() + 4 * ppo._offsets[k][0] for k in R.GNN_FLAT_ORDER)
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


def test_ten_updates_end_with_finite_changed_parameters():
    env, ppo = _trainer(True)                        # constructing this is the news: nothing fused accepted a GraphPolicy before
    assert ppo.gnn_hip_update and not ppo.hip_update
    before = ppo._flat.clone()
    obs = env.reset()["obs"]
    for _ in range(10):
        obs, last_value, _ = ppo.collect(obs)
        st = ppo.update(last_value)
        assert all(v == v for v in st.values()), st
    assert bool(torch.isfinite(ppo._flat).all()) and not torch.equal(before, ppo._flat)
    assert bool((ppo._flat != before).float().mean() > 0.5)      # every tensor moved, not one corner of the block
    env.close()
