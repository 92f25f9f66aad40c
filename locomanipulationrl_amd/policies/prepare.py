"""ctypes wrappers of the device-side preparation of a PPO iteration (csrc/lm_prepare.hip, include/lm_policy.h): pack_params = the parameter
block of a forward kernel packed from the flat block the optimiser steps (lm_mlp_pack_params / lm_gnn_pack_params: what pack_mlp_params /
pack_gnn_params build with torch), batch_stats = the sums both running scalers and the advantage normalisation need, batch_apply = the scaler
merge and the normalisation of the batch.  They launch on the current torch stream and never wait for the device.  No CPU fallback: a missing
library or a refused call raises with the reason."""
from __future__ import annotations

import ctypes as C

import torch

PACK_NONFINITE, PACK_RANGE = 1, 2      # bits of the pack status word (LM_PACK_* of include/lm_policy.h)


def _lib():
    from ..lib import load_library
    return load_library()


def _p(t):
    return C.c_void_p(None if t is None else t.data_ptr())


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _need_hip(dev, who):
    if dev.type != "cuda":
        raise RuntimeError(f"{who} runs on a HIP device only, not {dev} (no CPU fallback)")


def scaler_state(size: int, device):
    """A scaler state block: float64 [2 size + 1] = mean | var | count, initially 0, 1, 1 (RunningStandardScaler's initial state)."""
    st = torch.zeros(2 * size + 1, device=device, dtype=torch.float64)
    st[size:] = 1.0
    return st


def pack_status_error(status: int, kind: str):
    """The ValueError of the torch packers for a non-zero pack status word (None for 0)."""
    if not status:
        return None
    name = "MLP" if kind == "mlp" else "GNN"
    return ValueError(f"{name} weights must be finite and below the fp16 range (6e4) for the split-fp16 matrix products (pack status {int(status)}: "
                      f"{'a non-finite weight' if status & PACK_NONFINITE else ''}{'; ' if status == 3 else ''}{'|w| >= 6e4' if status & PACK_RANGE else ''})")


def pack_params(kind: str, flat, num_obs: int, packed, status, state=None, eps: float = 1e-8, clip: float = 5.0):
    """lm_mlp_pack_params (kind 'mlp') / lm_gnn_pack_params ('gnn'): one launch that fills `packed` (the forward kernel's block, e.g. a rollout
    plan's) from the flat fp32 block `flat` and the observation scaler's state block `state` (None: identity statistics), bit for bit what the
    torch packers build.  `status` is a device int32 the kernel ORs LM_PACK_* bits into instead of raising; nothing is read back here."""
    lib = _lib()
    dev = flat.device
    _need_hip(dev, "pack_params")
    fn, want_flat, want_packed = (lib.lm_mlp_pack_params, lib.lm_mlp_grad_param_count(int(num_obs)), lib.lm_mlp_param_count_obs(int(num_obs))) if kind == "mlp" else \
        (lib.lm_gnn_pack_params, lib.lm_gnn_grad_param_count(), lib.lm_gnn_param_count())
    assert flat.dtype == torch.float32 and flat.is_contiguous() and flat.numel() == want_flat, (flat.dtype, flat.numel(), want_flat)
    assert packed.device == dev and packed.dtype == torch.float32 and packed.is_contiguous() and packed.numel() == want_packed, (packed.numel(), want_packed)
    assert status.device == dev and status.dtype == torch.int32 and status.numel() == 1
    if state is not None:
        assert state.device == dev and state.dtype == torch.float64 and state.is_contiguous() and state.numel() == 2 * int(num_obs) + 1, tuple(state.shape)
    with torch.cuda.device(dev):            # the kernel launches on the calling thread's current device
        rc = fn(_p(flat), int(num_obs), _p(state), float(eps), float(clip), _p(packed), _p(status), _stream(dev))
    if rc != 0:
        raise RuntimeError(f"lm_{kind}_pack_params failed ({rc}): {lib.lm_last_error().decode()}")
    return packed


def batch_stats_workspace(B: int, C_: int, device):
    """A zeroed workspace of the size lm_ppo_batch_stats needs for B samples of C features (its first word is the kernel's ticket counter: zero
    before the first call, left zero by every call)."""
    lib = _lib()
    nbytes = lib.lm_ppo_batch_stats_workspace(int(B), int(C_))
    if nbytes <= 0:
        raise RuntimeError(f"lm_ppo_batch_stats_workspace failed ({nbytes}): {lib.lm_last_error().decode()}")
    return torch.zeros((nbytes + 7) // 8, device=device, dtype=torch.float64)


def batch_stats(obs, ret, adv, sums=None, workspace=None):
    """lm_ppo_batch_stats: sums = S obs_c | S obs_c^2 | S ret | S ret^2 | S adv | S adv^2 | B (float64 [2 C + 5]) of obs (B, C), ret (B,), adv (B,),
    accumulated in double in a fixed order.  `sums` and `workspace` are allocated when not given."""
    lib = _lib()
    dev = obs.device
    _need_hip(dev, "batch_stats")
    B, C_ = int(obs.shape[0]), int(obs.shape[1])
    for t, shape in ((obs, (B, C_)), (ret, (B,)), (adv, (B,))):
        assert t.device == dev and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape, (t.dtype, tuple(t.shape), shape)
    if sums is None: sums = torch.empty(2 * C_ + 5, device=dev, dtype=torch.float64)
    if workspace is None: workspace = batch_stats_workspace(B, C_, dev)
    assert sums.device == dev and sums.dtype == torch.float64 and sums.is_contiguous() and sums.numel() == 2 * C_ + 5 and workspace.device == dev
    with torch.cuda.device(dev):
        rc = lib.lm_ppo_batch_stats(_p(obs), _p(ret), _p(adv), B, C_, _p(sums), _p(workspace), workspace.numel() * workspace.element_size(), _stream(dev))
    if rc != 0:
        raise RuntimeError(f"lm_ppo_batch_stats failed ({rc}): {lib.lm_last_error().decode()}")
    return sums


def batch_apply(obs, ret, old_val, adv, sums, obs_state, val_state, freeze_obs=False, eps: float = 1e-8, clip: float = 5.0, out=None):
    """lm_ppo_batch_apply: merges `sums` into the two scaler state blocks (the observation scaler's is left alone under freeze_obs) as
    RunningStandardScaler.update does, then writes (obs_n, ret_n, old_val_n, adv_n) from the merged states.  out: the four output tensors to
    reuse (allocated when not given)."""
    lib = _lib()
    dev = obs.device
    _need_hip(dev, "batch_apply")
    B, C_ = int(obs.shape[0]), int(obs.shape[1])
    for t, shape in ((obs, (B, C_)), (ret, (B,)), (old_val, (B,)), (adv, (B,))):
        assert t.device == dev and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape, (t.dtype, tuple(t.shape), shape)
    for t, n in ((sums, 2 * C_ + 5), (obs_state, 2 * C_ + 1), (val_state, 3)):
        assert t.device == dev and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == n, (t.dtype, tuple(t.shape), n)
    if out is None:
        out = (torch.empty_like(obs), torch.empty_like(ret), torch.empty_like(old_val), torch.empty_like(adv))
    for o, t in zip(out, (obs, ret, old_val, adv)):
        assert o.device == dev and o.dtype == torch.float32 and o.is_contiguous() and tuple(o.shape) == tuple(t.shape)
    with torch.cuda.device(dev):
        rc = lib.lm_ppo_batch_apply(_p(obs), _p(ret), _p(old_val), _p(adv), B, C_, _p(sums), _p(obs_state), _p(val_state), int(bool(freeze_obs)), float(eps),
                                    float(clip), _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]), _stream(dev))
    if rc != 0:
        raise RuntimeError(f"lm_ppo_batch_apply failed ({rc}): {lib.lm_last_error().decode()}")
    return out
