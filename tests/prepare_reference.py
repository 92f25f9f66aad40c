"""Float64 reference of the device-side batch preparation (csrc/lm_prepare.hip), shared by tests/test_prepare_host.py and
tests/test_gpu_prepare.py: the scaler merge of train/ppo.py RunningStandardScaler.update from a block of sums, in plain Python floats (IEEE
doubles, one rounding per operation, the operation order of the class), and the normalisation of a batch from a merged state.  Host
arithmetic only."""
import math

import torch

EPS, CLIP = 1e-8, 5.0


def sums_of(obs, ret, adv):
    """The sums block of lm_ppo_batch_stats, exactly: math.fsum of the inputs as doubles (squares of fp32 values are exact in double).
    Returns (sums [2 C + 5], abs_sums [2 C + 4]): abs_sums = S |term| of each entry, the scale of the summation-order bound."""
    o, r, a = obs.double(), ret.double(), adv.double()
    B, C = o.shape
    cols = [o[:, c].tolist() for c in range(C)]
    lists = cols + [[x * x for x in col] for col in cols] + [r.tolist(), [x * x for x in r.tolist()], a.tolist(), [x * x for x in a.tolist()]]
    return [math.fsum(l) for l in lists] + [float(B)], [math.fsum(abs(x) for x in l) for l in lists]


def merge(mean, var, count, s, ss, n):
    """One feature of RunningStandardScaler.update in Python floats: (mean, var, count) after merging a batch with sum s, sum of squares ss, n rows."""
    bmean = s / n
    bvar = max(ss / n - bmean * bmean, 0.0) * n / max(n - 1.0, 1.0)
    delta = bmean - mean; tot = count + n
    m2 = var * count + bvar * n + delta * delta * count * n / tot
    return mean + delta * n / tot, m2 / tot, tot


def merge_state(state, s, ss, n):
    """state = [mean (C) | var (C) | count] as a list of floats -> the merged list."""
    C = (len(state) - 1) // 2
    out = [merge(state[c], state[C + c], state[2 * C], s[c], ss[c], n) for c in range(C)]
    return [m for m, _, _ in out] + [v for _, v, _ in out] + [out[0][2]]


def merge_sums(obs_state, val_state, sums, freeze_obs=False):
    """What lm_ppo_batch_apply's merge does to the two state blocks (lists of floats) for a sums block (list of floats)."""
    C = (len(sums) - 5) // 2
    n = sums[2 * C + 4]
    new_obs = list(obs_state) if freeze_obs else merge_state(obs_state, sums[:C], sums[C:2 * C], n)
    return new_obs, merge_state(val_state, [sums[2 * C]], [sums[2 * C + 1]], n)


def normalise64(x, mean, var, eps=EPS, clip=CLIP):
    """clamp((x - mean) / (sqrt(var) + eps), +-clip) in float64 tensors; also returns the bound's scale (|x| + |mean|) / (sqrt(var) + eps)."""
    x = x.double(); den = var.sqrt() + eps
    return ((x - mean) / den).clamp(-clip, clip), (x.abs() + mean.abs()) / den


def adv_stats(sums):
    """(mean, unbiased std) of the advantages from a sums block, in Python floats."""
    C = (len(sums) - 5) // 2
    n, sa, saa = sums[2 * C + 4], sums[2 * C + 2], sums[2 * C + 3]
    return sa / n, math.sqrt(max((saa - sa * sa / n) / (n - 1.0), 0.0))


def ulps64(a, b):
    """Distance of two doubles in units in the last place of the larger one."""
    if a == b:
        return 0.0
    return abs(a - b) / math.ulp(max(abs(a), abs(b)))


def make_batch(B, C, seed=0):
    """fp32 inputs in [-5, 5] for the statistics tests: column 1 a constant 0.5, column 2 all zero, column 3 mean 4 and spread 0.5."""
    g = torch.Generator().manual_seed(1000 * C + B + seed)
    obs = (torch.rand(B, C, generator=g) * 10 - 5).float()
    obs[:, 1] = 0.5; obs[:, 2] = 0.0
    obs[:, 3] = (4 + (torch.rand(B, generator=g) - 0.5)).float()
    ret = (torch.rand(B, generator=g) * 10 - 5).float(); adv = (torch.rand(B, generator=g) * 10 - 5).float()
    return obs, ret, adv
