"""Float64 reference of the gaussian action sampling (csrc/lm_policy_dev.h ro_normal / ro_key, csrc/lm_policy.hip k_sample_actions and the fused
epilogues of the policy tiles), restated in plain numpy from the formulas alone.  Imports nothing from the library: what it computes is pinned to
the oracle's lmo_dr_sample by tests/test_policy_reference_host.py before anything on the GPU is compared with it.

The per-element bounds of the GPU comparison live here too.  They are functions of the reference's values only."""
import math

import numpy as np

STREAM_ACTION_SAMPLING = 9          # csrc/lm_rng.h: streams 0..8 are the domain-randomisation channels
LN_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)
_M32 = np.uint64(0xFFFFFFFF)


def _u(x):
    """Integers (python ints, int64 or unsigned arrays) -> uint64 array holding the value modulo 2^32, as a C cast to uint32_t gives."""
    a = np.asarray(x)
    assert a.dtype.kind in "iu", a.dtype
    return a.astype(np.uint64) & _M32          # a negative int64 wraps to its two's complement: the low 32 bits are those of the C cast


def _mul(a, b):
    return (a * np.uint64(b)) & _M32          # both factors below 2^32: the uint64 product is exact


def mix32(x):
    """lowbias32 finaliser on uint64 arrays holding 32-bit values."""
    x = x & _M32
    x = x ^ (x >> np.uint64(16)); x = _mul(x, 0x7feb352d)
    x = x ^ (x >> np.uint64(15)); x = _mul(x, 0x846ca68b)
    return x ^ (x >> np.uint64(16))


def rng_base(seed, stream, env, key):
    """lm_rng_base: hash of (seed, stream, env, key)."""
    seed, stream, env, key = _u(seed), _u(stream), _u(env), _u(key)
    return mix32(seed ^ mix32((_mul(env, 0x9E3779B9) + np.uint64(0x7F4A7C15)) & _M32) ^ mix32((_mul(key, 0x85EBCA6B) + np.uint64(0x165667B1)) & _M32)
                 ^ mix32((_mul(stream, 0x27D4EB2F) + np.uint64(0x632BE5AB)) & _M32))


def rng_pair_bits(base, pair):
    """lm_rng_pair, the integer part: the two 24-bit integers (r1 >> 8, r2 >> 8) of pair `pair`."""
    pair = _u(pair)
    k1 = (np.uint64(2) * pair + np.uint64(1)) & _M32; k2 = (np.uint64(2) * pair + np.uint64(2)) & _M32
    r1 = mix32((base + _mul(k1, 0xC2B2AE35)) & _M32); r2 = mix32((base + _mul(k2, 0xC2B2AE35)) & _M32)
    return r1 >> np.uint64(8), r2 >> np.uint64(8)


def box_muller(seed, stream, env, key, pair, sine):
    """One standard normal in float64: radius from u1 = ((r1 >> 8) + 1) / 2^24 in (0, 1], angle 2 pi u2 with u2 = (r2 >> 8) / 2^24 in [0, 1);
    the sine branch where `sine` is non-zero, else the cosine branch.  All arguments broadcast."""
    i1, i2 = rng_pair_bits(rng_base(seed, stream, env, key), pair)
    u1 = (i1.astype(np.float64) + 1.0) / 16777216.0; u2 = i2.astype(np.float64) / 16777216.0
    rad = np.sqrt(-2.0 * np.log(u1)); ang = 2.0 * math.pi * u2
    return rad * np.where(np.asarray(sine) != 0, np.sin(ang), np.cos(ang))


def normal_ref(seed, env, key, idx):
    """ro_normal: stream 9; actions 2p and 2p + 1 are the cosine and the sine branch of pair p = idx >> 1."""
    idx = _u(idx)
    return box_muller(seed, STREAM_ACTION_SAMPLING, env, key, idx >> np.uint64(1), idx & np.uint64(1))


def key_ref(cnt, N, env):
    """ro_key: ((uint32(episode count) << 16) + uint32(progress_buf)) mod 2^32 from the engine's int64 [6][N] counter block (row 4 = progress_buf,
    row 5 = episode count).  uint64 array."""
    c = np.asarray(cnt, dtype=np.int64).reshape(6, N)
    env = np.asarray(env, dtype=np.int64)
    return ((_u(c[5][env]) << np.uint64(16)) + _u(c[4][env])) & _M32


def sample_ref(mean, log_std, cnt, seed):
    """(eps [N][12], actions [N][12], logp [N]) in float64: eps_j = normal_ref(seed, env, key(env), j), actions = mean + exp(ls) eps,
    logp = sum_j (-eps_j^2 / 2 - ls_j - ln sqrt(2 pi))."""
    mean = np.asarray(mean, dtype=np.float64); ls = np.asarray(log_std, dtype=np.float64).reshape(1, 12)
    N = mean.shape[0]
    assert mean.shape == (N, 12)
    env = np.arange(N, dtype=np.int64)
    key = key_ref(cnt, N, env)
    eps = normal_ref(seed, env[:, None], key[:, None], np.arange(12, dtype=np.int64)[None, :])
    return eps, mean + np.exp(ls) * eps, logp_terms(ls, eps).sum(1)


def logp_terms(log_std, eps):
    return -0.5 * eps * eps - np.asarray(log_std, dtype=np.float64).reshape(1, 12) - LN_SQRT_2PI


# ---- bounds of the fp32 device code against this reference, per element, from the reference's values only
# EPS_BOUND: the device draws in fp32.  The angle 6.2831855f * u2 carries at most 4.2e-7 rad (one fp32 rounding of a value below 2 pi plus the
# constant's error); sine and cosine at most 2 ulp of a value of magnitude at most 1 (1.2e-7); the radius is at most sqrt(-2 ln 2^-24) = 5.77
# with a relative error of at most 2e-7 from logf and sqrtf; the product's rounding 3.4e-7: together at most 4.3e-6.  1e-5 leaves a factor of two
# for the device's libm.
EPS_BOUND = 1e-5


def action_bound(mean, log_std, eps_ref):
    """|a_dev - a_ref| <= exp(ls) EPS_BOUND + 2^-22 (|mean| + exp(ls) |eps_ref|): the draw's error scaled by the standard deviation, plus expf
    (relative error of a few 2^-24 on the product) and the fma's one rounding of the result."""
    sd = np.exp(np.asarray(log_std, dtype=np.float64).reshape(1, 12))
    return sd * EPS_BOUND + 2.0 ** -22 * (np.abs(mean) + sd * np.abs(eps_ref))


def logp_bound(log_std, eps_ref):
    """|logp_dev - logp_ref| <= sum_j |eps_ref_j| EPS_BOUND + 6e-10 + 16 * 2^-24 sum_j |term_j|: the first-order effect of the draw's error on
    eps^2 / 2, its second-order effect (12 EPS_BOUND^2 / 2), and twelve fp32 terms of three to four roundings each plus the grouped sum."""
    return np.abs(eps_ref).sum(1) * EPS_BOUND + 6e-10 + 16.0 * 2.0 ** -24 * np.abs(logp_terms(log_std, eps_ref)).sum(1)


# ---- synthetic counter blocks for lm_sample_actions
EDGE_PAIRS = ((0, 0), (0, 1), (1, 0), (0, 65535), (0, 65536), (65535, 65535), (65536, 5), (2 ** 32 + 3, 7))      # (episode count, progress_buf)


def synthetic_counters(N, rng):
    """int64 [6][N]: the first envs carry EDGE_PAIRS, the others a random episode count in [0, 70000) and progress in [0, 1000); rows 0..3 hold
    a sentinel pattern (large, different in every row and env) so that a wrong row index gives another key."""
    cnt = np.empty((6, N), dtype=np.int64)
    for r in range(4):
        cnt[r] = 0x5A5A0000 + 0x01010101 * (r + 1) + 7919 * np.arange(N, dtype=np.int64)
    cnt[5] = rng.integers(0, 70000, size=N); cnt[4] = rng.integers(0, 1000, size=N)
    for i, (ep, pr) in enumerate(EDGE_PAIRS[:N]):
        cnt[5, i] = ep; cnt[4, i] = pr
    return cnt
