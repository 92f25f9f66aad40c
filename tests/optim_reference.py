"""Float64 reference of the device optimiser step (lm_adam_clip_step, lm_kl_adaptive_lr; csrc/lm_optim.hip), written from the formulas of
include/lm_policy.h and not by calling torch's optimiser, the inputs its tests share, and torch's own clip_grad_norm_ + Adam on the CPU (in
float64 to pin the reference, in float32 as the yardstick of what fp32 delivers).  CPU only; nothing here touches the library."""
import functools
import math

import numpy as np
import torch

HYPER = dict(lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=1.0)
STEPS = 3
SIZES = (1, 3, 63, 64, 65, 1025, 10190, 58649, 64793)      # around the 16-byte vector, the 64-lane workgroup, several workgroups, and the three flat blocks
SCALES = ("below", "above", "zero", "sparse")                # gradient norm below the clip | 50 x above it | all zeros | every third entry zero, non-zero moments


def clip_adam_step64(p, g, m, v, step, lr, beta1, beta2, eps, max_norm, clamp=None):
    """One step in float64.  p, g, m, v: 1-D tensors (any float dtype; converted); clamp = (offset, count, minimum) or None.
    Returns (p, m, v, step, norm, coef), new float64 tensors and Python floats."""
    p, g, m, v = (x.detach().double().clone() for x in (p, g, m, v))
    norm = math.sqrt(float((g * g).sum()))
    coef = min(1.0, max_norm / (norm + 1e-6))
    g = coef * g
    step = step + 1
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    p = p - (lr / (1.0 - beta1 ** step)) * m / (v.sqrt() / math.sqrt(1.0 - beta2 ** step) + eps)
    if clamp is not None:
        o, c, lo = clamp
        p[o:o + c] = p[o:o + c].clamp_min(lo)
    return p, m, v, step, norm, coef


def kl_rule(lr, kls, thr, lr_min, lr_max):
    """The KL-adaptive rate: the mean of `kls` (summed in double, in order) against the thresholds; returns the new rate."""
    s = 0.0
    for k in kls:
        s += float(k)
    kl = s / len(kls)
    if thr > 0:
        if kl > 2 * thr:
            lr = max(lr / 1.5, lr_min)
        elif kl < thr / 2:
            lr = min(lr * 1.5, lr_max)
    return lr


def torch_steps(p, grads, m, v, dtype, lr, beta1, beta2, eps, max_norm):
    """torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on the CPU in `dtype` over the gradients `grads`, from the moments (m, v) at step 0.
    Returns the list of (p, m, v) after each step."""
    q = torch.nn.Parameter(p.detach().to(dtype).clone())
    opt = torch.optim.Adam([q], lr=lr, betas=(beta1, beta2), eps=eps)
    opt.state[q] = {"step": torch.tensor(0.0), "exp_avg": m.detach().to(dtype).clone(), "exp_avg_sq": v.detach().to(dtype).clone()}
    out = []
    for g in grads:
        q.grad = g.detach().to(dtype).clone()
        torch.nn.utils.clip_grad_norm_([q], max_norm)
        opt.step()
        out.append((q.detach().clone(), opt.state[q]["exp_avg"].clone(), opt.state[q]["exp_avg_sq"].clone()))
    return out


def rel(x, ref):
    """||x - ref|| / ||ref||; a zero reference demands exact zeros."""
    x, ref = x.double(), ref.double()
    e, r = float((x - ref).norm()), float(ref.norm())
    return e / r if r > 0 else (0.0 if e == 0 else float("inf"))


class Case:
    pass


@functools.lru_cache(maxsize=None)
def make_case(n, scale):
    """float32 inputs of one (n, scale) case: parameters, moments at step 0 and STEPS gradients.  Computed once, never modified."""
    g = torch.Generator().manual_seed(7919 * n + SCALES.index(scale))
    c = Case(); c.n, c.scale = n, scale
    c.p = torch.randn(n, generator=g)
    if scale == "zero":
        c.m, c.v = torch.zeros(n), torch.zeros(n)
        c.grads = [torch.zeros(n) for _ in range(STEPS)]
        return c
    c.m = 0.02 * torch.randn(n, generator=g); c.v = (0.02 * torch.randn(n, generator=g)) ** 2
    c.grads = []
    for _ in range(STEPS):
        x = torch.randn(n, generator=g)
        if scale == "sparse" and n >= 3:
            x[::3] = 0.0
        target = {"below": 0.5, "sparse": 0.5, "above": 50.0}[scale] * HYPER["max_norm"]
        c.grads.append((x.double() * (target / float(x.double().norm()))).float())
    return c


@functools.lru_cache(maxsize=None)
def reference(n, scale):
    """(case, float64 trajectory, fp32 errors): the trajectory is [(p, m, v, step, norm, coef)] after each step; the errors are torch's own
    fp32 clip + Adam on the CPU against it after the last step, per buffer, with the parameters measured by their change."""
    c = make_case(n, scale)
    h = HYPER
    traj, p, m, v, step = [], c.p, c.m, c.v, 0
    for g in c.grads:
        p, m, v, step, norm, coef = clip_adam_step64(p, g, m, v, step, h["lr"], h["beta1"], h["beta2"], h["eps"], h["max_norm"])
        traj.append((p, m, v, step, norm, coef))
    p32, m32, v32 = torch_steps(c.p, c.grads, c.m, c.v, torch.float32, **h)[-1]
    return c, traj, buffer_errors(c, traj, p32, m32, v32)


def buffer_errors(c, traj, p, m, v):
    p64, m64, v64 = traj[-1][:3]
    return {"exp_avg": rel(m, m64), "exp_avg_sq": rel(v, v64), "delta_p": rel(p.double() - c.p.double(), p64 - c.p.double())}


@functools.lru_cache(maxsize=None)
def yardstick():
    """e_t per buffer: the largest error of torch's fp32 over the whole case list (the convention of DESIGN.md 5.4)."""
    e = {"exp_avg": 0.0, "exp_avg_sq": 0.0, "delta_p": 0.0}
    for n in SIZES:
        for s in SCALES:
            for k, x in reference(n, s)[2].items():
                e[k] = max(e[k], x)
    return e


def _f32_next(x, up):
    return float(np.nextafter(np.float32(x), np.float32(np.inf if up else -np.inf)))


THR = 2.0 ** -6      # 2 thr and thr / 2 are exact in fp32, the type the KL values have on the device


def kl_table():
    """[(name, lr, [one KL value per call], thr, lr_min, lr_max, expectation)] with every KL an fp32 value; expectation per call: -1 the rate
    goes down, 0 it stays, +1 it goes up, None not stated (where the rate walks into a bound)."""
    lr, lo, hi = 3e-4, 1e-6, 1e-2
    t = [("at 2 thr", lr, [2 * THR], THR, lo, hi, [0]), ("at thr / 2", lr, [THR / 2], THR, lo, hi, [0]),
         ("just above 2 thr", lr, [_f32_next(2 * THR, True)], THR, lo, hi, [-1]), ("just below 2 thr", lr, [_f32_next(2 * THR, False)], THR, lo, hi, [0]),
         ("just above thr / 2", lr, [_f32_next(THR / 2, True)], THR, lo, hi, [0]), ("just below thr / 2", lr, [_f32_next(THR / 2, False)], THR, lo, hi, [1]),
         # the recipe's threshold is no fp32 value: its two fp32 neighbours
         ("recipe, above", lr, [_f32_next(0.024, True)], 0.012, lo, hi, [-1]), ("recipe, below", lr, [_f32_next(0.006, False)], 0.012, lo, hi, [1]),
         ("walk into lr_min", lr, [float(np.float32(0.5))] * 20, THR, lo, hi, None), ("walk into max_lr", lr, [0.0] * 12, THR, lo, hi, None),
         ("thr 0, high", lr, [float(np.float32(0.5))], 0.0, lo, hi, [0]), ("thr 0, low", lr, [0.0], 0.0, lo, hi, [0])]
    return t


def spread3(kl):
    """Three fp32 values around `kl` whose double mean is what the device takes for count = 3."""
    return [float(np.float32(kl * f)) for f in (0.9, 1.0, 1.1)]
