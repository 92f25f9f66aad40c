"""MLP policy of the reference's PPO scripts (scripts/skrl_ppo_locomotion.py:25-52): shared trunk 64-256-128-64 (ELU),
Gaussian mean head (12), value head (1), log-std parameter; plus the matrix-core forward for rollouts with skrl's
RunningStandardScaler observation preprocessor folded in (:96-99).  The forward computes its fp32 products on the fp16 matrix pipe with every
operand split into two fp16 halves (fp32-level accuracy): the weights are split here, on the host (`_pack_q`)."""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn


class SharedMLP(nn.Module):
    def __init__(self, num_observations=64, num_actions=12):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(num_observations, 256), nn.ELU(), nn.Linear(256, 128), nn.ELU(), nn.Linear(128, 64), nn.ELU())
        self.mean_layer = nn.Linear(64, num_actions)
        self.log_std_parameter = nn.Parameter(torch.zeros(num_actions))
        self.value_layer = nn.Linear(64, 1)
        self._packed = None

    def forward(self, obs):
        h = self.net(obs)
        return self.mean_layer(h), self.log_std_parameter, self.value_layer(h)

    @torch.no_grad()
    def act_inference(self, obs, obs_mean=None, obs_var=None, eps=1e-8, clip=5.0):
        if self._packed is None or self._packed.device != obs.device:
            self.refresh(obs.device, obs_mean, obs_var, eps, clip)
        mean, value = mlp_forward_hip(obs, self._packed)
        return mean, self.log_std_parameter, value

    def refresh(self, device=None, obs_mean=None, obs_var=None, eps=1e-8, clip=5.0):
        self._packed = pack_mlp_params(self, obs_mean, obs_var, eps, clip).to(device or self.log_std_parameter.device)


def _pack_q(W: torch.Tensor, natural_k: bool) -> torch.Tensor:
    """(out, in) fp32 weight -> the 32-bit words [out/16][KB][64 lanes][8] the MLP tile reads (csrc/lm_policy_dev.h): for output block mb,
    K-block kb (32 input features) and lane l = n + 16 g, the eight weights W[16 mb + n][col(kb, g, e)], e = 0..7, each split into two fp16
    halves (w = hi + lo, hi = fp16(w), lo = fp16(w - hi)): words 0..3 hold the hi halves (two per word, even e in the low 16 bits), words 4..7
    the lo halves.  col = 32 kb + 8 g + e for an input in natural order (the observation; columns beyond `in` are zero: 88 pads to 96), and
    16 (2 kb + (e >> 2)) + 4 g + (e & 3) for an input that is a previous layer's accumulator tile."""
    out_f, in_f = W.shape
    KB = (in_f + 31) // 32
    Wp = torch.zeros(out_f, 32 * KB, dtype=torch.float32, device=W.device); Wp[:, :in_f] = W.float()
    lane = torch.arange(64, device=W.device); n, g = lane & 15, lane >> 4
    mb = torch.arange(out_f // 16, device=W.device).view(-1, 1, 1, 1); kb = torch.arange(KB, device=W.device).view(1, -1, 1, 1)
    e = torch.arange(8, device=W.device).view(1, 1, 1, -1); nn, gg = n.view(1, 1, -1, 1), g.view(1, 1, -1, 1)
    row = (16 * mb + nn).expand(-1, KB, -1, 8)
    col = (32 * kb + 8 * gg + e) if natural_k else (16 * (2 * kb + (e >> 2)) + 4 * gg + (e & 3))
    w = Wp[row, col.expand(out_f // 16, -1, -1, -1)]                                   # [mb][kb][lane][e]
    if not bool(torch.isfinite(w).all()) or float(w.abs().max()) >= 6.0e4:
        raise ValueError("MLP weights must be finite and below the fp16 range (6e4) for the split-fp16 matrix products")
    hi = w.half(); lo = (w - hi.float()).half()                                          # round to nearest even, like the device's v_cvt_pk_f16_f32
    def pairs(h):                                                                        # fp16 [.., 8] -> int32 [.., 4]: even e in the low half
        u = h.view(torch.int16).to(torch.int32) & 0xFFFF
        return u[..., 0::2] | (u[..., 1::2] << 16)
    words = torch.cat([pairs(hi), pairs(lo)], dim=-1).contiguous()                       # [mb][kb][lane][8]
    return words.view(torch.float32).reshape(-1)                                         # bit patterns in a float32 tensor (never used as numbers)


def pack_mlp_params(m: SharedMLP, obs_mean=None, obs_var=None, eps=1e-8, clip=5.0) -> torch.Tensor:
    dev = m.log_std_parameter.device
    nobs = m.net[0].in_features
    assert nobs in (64, 88), "the MFMA forward is built for the 64- and 88-wide observations"
    mean = torch.zeros(nobs, device=dev) if obs_mean is None else obs_mean.detach().float().to(dev)
    # RunningStandardScaler: (x - mean) / (sqrt(var) + eps), then clamp(+-clip); identity statistics when absent
    istd = torch.ones(nobs, device=dev) if obs_var is None else 1.0 / (obs_var.detach().float().to(dev).sqrt() + eps)
    clipv = torch.tensor([clip if obs_var is not None else 3.0e38, 0, 0, 0], device=dev, dtype=torch.float32)
    l1, l2, l3 = m.net[0], m.net[2], m.net[4]
    Wh = torch.zeros(16, 64, device=dev); Wh[:12] = m.mean_layer.weight.detach(); Wh[12] = m.value_layer.weight.detach()[0]
    bh = torch.zeros(16, device=dev); bh[:12] = m.mean_layer.bias.detach(); bh[12] = m.value_layer.bias.detach()[0]
    parts = [mean, istd, clipv, _pack_q(l1.weight.detach(), True), l1.bias.detach(), _pack_q(l2.weight.detach(), False), l2.bias.detach(),
             _pack_q(l3.weight.detach(), False), l3.bias.detach(), _pack_q(Wh, False), bh]
    return torch.cat([p.reshape(-1).float() for p in parts]).contiguous()


def mlp_forward_hip(obs: torch.Tensor, packed: torch.Tensor):
    from ..lib import load_library
    lib = load_library()
    assert obs.is_cuda and obs.dtype == torch.float32 and obs.is_contiguous() and obs.shape[1] in (64, 88)
    assert packed.device == obs.device and packed.dtype == torch.float32 and packed.is_contiguous() and packed.numel() == lib.lm_mlp_param_count_obs(obs.shape[1])
    B = obs.shape[0]
    mean = torch.empty((B, 12), device=obs.device); value = torch.empty((B, 1), device=obs.device)
    with torch.cuda.device(obs.device):            # the kernel launches on the calling thread's current device
        rc = lib.lm_mlp_forward_obs(C.c_void_p(obs.data_ptr()), B, obs.shape[1], C.c_void_p(packed.data_ptr()), C.c_void_p(mean.data_ptr()),
                                C.c_void_p(value.data_ptr()), C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"lm_mlp_forward failed ({rc})")
    return mean, value


# ------------------------------------------------------------------------------------------------ PPO update on the GPU (csrc/lm_ppo.hip)
# names of SharedMLP's parameters in the order of the flat block of include/lm_policy.h (lm_mlp_ppo_grad)
FLAT_ORDER = ("net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias", "mean_layer.weight", "mean_layer.bias",
              "value_layer.weight", "value_layer.bias", "log_std_parameter")


def flatten_mlp_params(model: SharedMLP):
    """{parameter name: (offset, shape)} of the flat parameter / gradient block lm_mlp_ppo_grad reads and writes, and its length
    (= lm_mlp_grad_param_count(num_obs)).  Host arithmetic only: no library, no device."""
    named = dict(model.named_parameters())
    assert set(named) == set(FLAT_ORDER), sorted(named)
    offsets, o = {}, 0
    for name in FLAT_ORDER:
        offsets[name] = (o, tuple(named[name].shape)); o += named[name].numel()
    return offsets, o


@torch.no_grad()
def bind_flat_params(model: SharedMLP):
    """Move the model's parameters into ONE flat fp32 buffer in the header's order and their .grads into a second one: every parameter
    (and its .grad) becomes a view, so the kernel reads the weights the optimiser has just stepped and writes the gradient the optimiser
    reads next, with no copy in between.  state_dict() / load_state_dict() are unaffected (they copy values in place).  Returns
    (flat, grad_flat, offsets)."""
    offsets, total = flatten_mlp_params(model)
    named = dict(model.named_parameters())
    dev = model.log_std_parameter.device
    flat = torch.empty(total, device=dev, dtype=torch.float32); gflat = torch.zeros(total, device=dev, dtype=torch.float32)
    for name, (o, shape) in offsets.items():
        p = named[name]
        flat[o:o + p.numel()].copy_(p.detach().reshape(-1))
        p.data = flat[o:o + p.numel()].view(shape)
        p.grad = gflat[o:o + p.numel()].view(shape)
    return flat, gflat, offsets


def ppo_grad_geometry(num_obs: int, B: int, device=None):
    """(tile, groups): the sample-tile size and the number of workgroups lm_mlp_ppo_grad launches for B samples on `device`."""
    from ..lib import load_library
    lib = load_library(); tile, groups = C.c_int(0), C.c_int(0)
    with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
        rc = lib.lm_mlp_ppo_grad_geometry(int(num_obs), int(B), C.byref(tile), C.byref(groups))
    if rc != 0:
        raise RuntimeError(f"lm_mlp_ppo_grad_geometry failed ({rc}): {lib.lm_last_error().decode()}")
    return tile.value, groups.value


def ppo_grad_workspace(num_obs: int, B: int, device):
    """A workspace tensor of the size lm_mlp_ppo_grad needs for B samples (its contents never matter)."""
    from ..lib import load_library
    lib = load_library()
    with torch.cuda.device(device):
        nbytes = lib.lm_mlp_ppo_grad_workspace(int(num_obs), int(B))
    if nbytes <= 0:
        raise RuntimeError(f"lm_mlp_ppo_grad_workspace failed ({nbytes}): {lib.lm_last_error().decode()}")
    return torch.empty(nbytes // 4, device=device, dtype=torch.float32)


def mlp_ppo_grad(params, obs_n, actions, old_logp, old_value_n, adv, ret_n, ratio_clip=0.2, value_clip=0.2, value_scale=1.0, entropy_scale=0.0,
                 grad=None, stats=None, workspace=None):
    """lm_mlp_ppo_grad: loss and gradient of one PPO mini-batch for the flat SharedMLP parameter block `params` (order: FLAT_ORDER).
    Returns (grad, stats) with stats = [loss_pi, loss_v, kl, entropy term]; `grad`, `stats` and `workspace` are allocated when not given.
    No fallback: a missing kernel or a refused call raises."""
    from ..lib import load_library, LmPpoHyper
    lib = load_library()
    B, nobs = int(obs_n.shape[0]), int(obs_n.shape[1])
    dev = params.device
    if dev.type != "cuda":
        raise RuntimeError("mlp_ppo_grad runs on a HIP device only (no CPU fallback)")
    f32 = lambda t: t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()
    obs_n, actions, old_logp, old_value_n, adv, ret_n = (f32(t) for t in (obs_n, actions, old_logp, old_value_n, adv, ret_n))
    for t, shape in ((obs_n, (B, nobs)), (actions, (B, 12)), (old_logp, (B,)), (old_value_n, (B,)), (adv, (B,)), (ret_n, (B,))):
        assert t.device == dev and tuple(t.shape) == shape, (t.device, tuple(t.shape), shape)
    assert params.dtype == torch.float32 and params.is_contiguous() and params.numel() == lib.lm_mlp_grad_param_count(nobs), (params.numel(), nobs)
    if grad is None: grad = torch.empty_like(params)
    if stats is None: stats = torch.empty(4, device=dev, dtype=torch.float32)
    if workspace is None: workspace = ppo_grad_workspace(nobs, B, dev)
    assert grad.is_contiguous() and grad.numel() == params.numel() and stats.numel() == 4 and workspace.device == dev
    hp = LmPpoHyper(float(ratio_clip), float(value_clip), float(value_scale), float(entropy_scale))
    p = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):            # the kernels launch on the calling thread's current device
        rc = lib.lm_mlp_ppo_grad(p(params), p(obs_n), p(actions), p(old_logp), p(old_value_n), p(adv), p(ret_n), B, nobs, C.byref(hp), p(grad), p(stats),
                                 p(workspace), workspace.numel() * workspace.element_size(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"lm_mlp_ppo_grad failed ({rc}): {lib.lm_last_error().decode()}")
    return grad, stats


def gae(rewards, values, dones, last_value, gamma: float = 0.99, lam: float = 0.95):
    """lm_gae: (returns, advantages) of distributed.compute_gae, bit for bit, in one launch.  rewards / values (T, N) float32, dones (T, N)
    int64 (the rollout plan's own buffer), last_value (N,)."""
    from ..lib import load_library
    lib = load_library()
    dev = rewards.device
    if dev.type != "cuda":
        raise RuntimeError("gae runs on a HIP device only (distributed.compute_gae is the torch path)")
    T, N = rewards.shape
    assert dones.dtype == torch.int64 and tuple(dones.shape) == (T, N) and tuple(values.shape) == (T, N) and last_value.numel() == N
    rewards, values, dones, last_value = rewards.contiguous(), values.contiguous(), dones.contiguous(), last_value.contiguous()
    assert rewards.dtype == values.dtype == last_value.dtype == torch.float32
    ret = torch.empty((T, N), device=dev, dtype=torch.float32); adv = torch.empty((T, N), device=dev, dtype=torch.float32)
    p = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        rc = lib.lm_gae(p(rewards), p(values), p(dones), p(last_value), int(T), int(N), float(gamma), float(lam), p(ret), p(adv),
                        C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"lm_gae failed ({rc}): {lib.lm_last_error().decode()}")
    return ret, adv
