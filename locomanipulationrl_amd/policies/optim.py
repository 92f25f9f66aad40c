"""ctypes wrappers of the optimiser step of the PPO update (csrc/lm_optim.hip, include/lm_policy.h): lm_adam_clip_step = clip_grad_norm_ + Adam on
one flat fp32 block, lm_kl_adaptive_lr = the KL-adaptive rate, and the device-resident state block the two share.  They launch on the current
torch stream and never wait for the device.  No CPU fallback: a missing library or a refused call raises with the reason."""
from __future__ import annotations

import ctypes as C

import torch

# slots of the state block (LM_OPTIM_* of include/lm_policy.h)
STATE = dict(lr=0, step=1, grad_norm=2, clip_coef=3, kl=4)


def _lib():
    from ..lib import load_library
    return load_library()


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _check_state(state):
    if state.device.type != "cuda":
        raise RuntimeError("the optimiser state block lives on a HIP device (no CPU fallback)")
    assert state.dtype == torch.float64 and state.is_contiguous() and state.numel() == _lib().lm_optim_state_len(), (state.dtype, tuple(state.shape))


def optim_state(device, lr: float, step: int = 0, state=None):
    """lm_optim_state_init: the state block (a float64 device tensor of lm_optim_state_len() slots: STATE) with the given rate and step
    count, clip_coef 1 and the rest 0.  `state`: an existing block to reset in place (allocated when not given)."""
    lib = _lib()
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"optim_state needs a HIP device, not {dev} (the optimiser kernels have no CPU fallback)")
    if state is None:
        state = torch.zeros(lib.lm_optim_state_len(), device=dev, dtype=torch.float64)
    _check_state(state)
    with torch.cuda.device(state.device):
        rc = lib.lm_optim_state_init(_p(state), float(lr), float(step), _stream(state.device))
    if rc != 0:
        raise RuntimeError(f"lm_optim_state_init failed ({rc}): {lib.lm_last_error().decode()}")
    return state


def adam_clip_step(params, grad, exp_avg, exp_avg_sq, state, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=1.0, clamp=None):
    """lm_adam_clip_step: one clip_grad_norm_(max_norm) + Adam step on the flat fp32 block `params` with the rate in `state`; `grad` is read
    only, the moments and `state` (step, grad_norm, clip_coef) are updated in place.  clamp = (offset, count, minimum) floors that range of
    `params` after the step."""
    from ..lib import LmOptimHyper
    lib = _lib()
    dev = params.device
    if dev.type != "cuda":
        raise RuntimeError("adam_clip_step runs on a HIP device only (no CPU fallback)")
    n = params.numel()
    for t in (params, grad, exp_avg, exp_avg_sq):
        assert t.device == dev and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n, (t.device, t.dtype, tuple(t.shape), n)
    _check_state(state)
    assert state.device == dev
    off, cnt, cmin = (0, 0, 0.0) if clamp is None else clamp
    hp = LmOptimHyper(float(beta1), float(beta2), float(eps), float(max_norm), int(off), int(cnt), float(cmin), 0)
    with torch.cuda.device(dev):            # the kernels launch on the calling thread's current device
        rc = lib.lm_adam_clip_step(_p(params), _p(grad), _p(exp_avg), _p(exp_avg_sq), int(n), _p(state), C.byref(hp), _stream(dev))
    if rc != 0:
        raise RuntimeError(f"lm_adam_clip_step failed ({rc}): {lib.lm_last_error().decode()}")


def kl_adaptive_lr(state, kl, threshold: float, lr_min: float = 1e-6, lr_max: float = 1e-2):
    """lm_kl_adaptive_lr: the mean of the fp32 device values `kl` (summed in double) moves state's rate by the rule of PPO.update; the mean is
    left in state (STATE['kl'])."""
    lib = _lib()
    _check_state(state)
    dev = state.device
    assert kl.device == dev and kl.dtype == torch.float32 and kl.numel() >= 1 and (kl.numel() == 1 or kl.is_contiguous()), (kl.device, kl.dtype, tuple(kl.shape))
    with torch.cuda.device(dev):
        rc = lib.lm_kl_adaptive_lr(_p(state), _p(kl), int(kl.numel()), float(threshold), float(lr_min), float(lr_max), _stream(dev))
    if rc != 0:
        raise RuntimeError(f"lm_kl_adaptive_lr failed ({rc}): {lib.lm_last_error().decode()}")
