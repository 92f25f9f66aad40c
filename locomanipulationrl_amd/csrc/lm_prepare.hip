// lm_prepare.hip -- what a PPO iteration does around the rollout and the epoch loop, on the device (include/lm_policy.h): the parameter pack of the
// two forward kernels from the flat fp32 block the optimiser steps (lm_mlp_pack_params, lm_gnn_pack_params), the batch statistics of the two
// running scalers and of the advantage normalisation (lm_ppo_batch_stats), and the scaler merge plus the normalisation of the batch
// (lm_ppo_batch_apply).  None of them waits for the host, allocates or synchronises; the range check of the packers becomes a status word.
//
// Launches, and why none of them can race:
//   k_pack_mlp / k_pack_gnn   one launch, one thread per output word; reads flat and the scaler state, writes packed; ORs the status word with an
//                             integer atomic (OR is order-free: the word is the same whatever order the lanes arrive in).
//   k_prep_stats              ONE launch.  Every workgroup writes its partial sums (double) to its own row of the workspace, publishes them with a
//                             device-scope fence and takes a ticket from an integer counter; the workgroup that draws the last ticket adds the
//                             rows in row order - an order fixed by (B, C) alone - and writes `sums`.  No floating-point atomics: which workgroup
//                             happens to run the final pass does not change a bit of it.  The counter is left 0 for the next call.
//   k_prep_merge              ONE workgroup.  The only writer of the two scaler states; reads `sums`.
//   k_prep_apply              many workgroups.  Reads the two states and `sums`, writes the four normalised outputs, writes no state.
// A scaler state is thus written by a launch of one workgroup and read by a later launch, as state[] of csrc/lm_optim.hip is.
// Arithmetic: double throughout, no contraction (the merge reproduces RunningStandardScaler.update operation for operation); the outputs are
// rounded to fp32 once.  The istd row of the packers is torch's fp32 expression 1 / (sqrt(float(var)) + float(eps)): each step is evaluated in
// double on fp32 operands and rounded to fp32, which is the correctly rounded fp32 result (53 >= 2 x 24 + 2), because plain fp32 sqrt and
// division in this library are 1-ulp approximations (lib.hipcc_command).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/lm_policy.h"
#include "../../include/lm_engine.h"
#include "lm_internal.h"

#pragma clang fp contract(off)

typedef float prep_f4 __attribute__((ext_vector_type(4)));

#define PREP_THREADS 256
#define PREP_MAX_GROUPS 512      // rows of partial sums the final pass adds: two waves of workgroups on 256 compute units
#define PREP_MIN_ROWS 64         // samples per workgroup below which another workgroup does not pay
#define PREP_WS_HEADER 16        // bytes: the ticket counter (int32) and padding, in front of the partial sums

// ------------------------------------------------------------------------------------------------ the packers
__device__ __forceinline__ float prep_istd(double var, float epsf) {
  const float vf = (float)var;
  const float s = (float)sqrt((double)vf);      // correctly rounded fp32 sqrt
  const float t = s + epsf;                     // one fp32 add, as torch's
  return (float)(1.0 / (double)t);              // correctly rounded fp32 reciprocal
}

__device__ __forceinline__ int prep_flags(float w) {
  const float a = __builtin_fabsf(w);
  if (!(a < __builtin_inff())) return LM_PACK_NONFINITE;      // inf or NaN
  return a >= 6.0e4f ? LM_PACK_RANGE : 0;
}

__device__ __forceinline__ uint32_t prep_half_bits(float x) { return (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)x); }   // round to nearest even

// the scaler rows both packers end / begin with: mean (n) | istd (n) | clip.  i in [0, 2 n]
__device__ __forceinline__ float prep_scaler_word(const double* __restrict__ st, int n, int i, float epsf, float clipf) {
  if (i < n) return st ? (float)st[i] : 0.0f;
  if (i < 2 * n) return st ? prep_istd(st[i], epsf) : 1.0f;      // st[n + c] is var[c]
  return st ? clipf : 3.0e38f;
}

// One 32-bit word of a split-fp16 weight block [out/16][KB][64 lanes][8] (policies/mlp_model.py _pack_q, csrc/lm_policy_dev.h): words 0..3 of a
// lane hold the hi halves of its eight weights, words 4..7 the lo halves, two per word with the even one in the low 16 bits.  W is (rows, in_f)
// row-major; rows at and beyond `rows` and columns at and beyond in_f read as 0; row `rows` reads Wx (the value head under the mean head) when
// given.  The hi word of a weight carries its range check.
__device__ __forceinline__ uint32_t prep_qword(const float* __restrict__ W, const float* __restrict__ Wx, int rows, int in_f, int KB, bool natural_k, int idx,
                                               int& flags) {
  const int j = idx & 7, lane = (idx >> 3) & 63, blk = idx >> 9, kb = blk % KB, mb = blk / KB;
  const int n = lane & 15, g = lane >> 4, row = 16 * mb + n;
  uint32_t word = 0;
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const int e = 2 * (j & 3) + h;
    const int col = natural_k ? 32 * kb + 8 * g + e : 16 * (2 * kb + (e >> 2)) + 4 * g + (e & 3);
    float w = 0.0f;
    if (col < in_f) {
      if (row < rows) w = W[row * in_f + col];
      else if (row == rows && Wx) w = Wx[col];
    }
    const _Float16 hi = (_Float16)w;
    uint32_t u;
    if (j < 4) { flags |= prep_flags(w); u = (uint32_t)__builtin_bit_cast(unsigned short, hi); }
    else u = prep_half_bits(w - (float)hi);
    word |= u << (16 * h);
  }
  return word;
}

__global__ void __launch_bounds__(PREP_THREADS) k_pack_mlp(const float* __restrict__ flat, int nobs, const double* __restrict__ st, float epsf, float clipf,
                                                           uint32_t* __restrict__ packed, int total, int32_t* status) {
  int i = blockIdx.x * PREP_THREADS + threadIdx.x;
  if (i >= total) return;
  const int out = i, kpad = (nobs + 31) & ~31;
  // flat block: W1 (256, nobs) | b1 | W2 (128, 256) | b2 | W3 (64, 128) | b3 | Wm (12, 64) | bm | Wv (1, 64) | bv | log_std
  const int f_b1 = 256 * nobs, f_w2 = f_b1 + 256, f_b2 = f_w2 + 128 * 256, f_w3 = f_b2 + 128, f_b3 = f_w3 + 64 * 128, f_wm = f_b3 + 64, f_bm = f_wm + 12 * 64,
            f_wv = f_bm + 12, f_bv = f_wv + 64;
  int flags = 0; uint32_t word;
  if (i < 2 * nobs + 4) {
    word = i <= 2 * nobs ? __builtin_bit_cast(uint32_t, prep_scaler_word(st, nobs, i, epsf, clipf)) : 0u;      // clip | 3 words of padding
  } else if ((i -= 2 * nobs + 4) < 256 * kpad) word = prep_qword(flat, nullptr, 256, nobs, kpad / 32, true, i, flags);
  else if ((i -= 256 * kpad) < 256) word = __builtin_bit_cast(uint32_t, flat[f_b1 + i]);
  else if ((i -= 256) < 128 * 256) word = prep_qword(flat + f_w2, nullptr, 128, 256, 8, false, i, flags);
  else if ((i -= 128 * 256) < 128) word = __builtin_bit_cast(uint32_t, flat[f_b2 + i]);
  else if ((i -= 128) < 64 * 128) word = prep_qword(flat + f_w3, nullptr, 64, 128, 4, false, i, flags);
  else if ((i -= 64 * 128) < 64) word = __builtin_bit_cast(uint32_t, flat[f_b3 + i]);
  else if ((i -= 64) < 16 * 64) word = prep_qword(flat + f_wm, flat + f_wv, 12, 64, 2, false, i, flags);      // rows 0..11 mean, 12 value, 13..15 zero
  else { i -= 16 * 64; word = i < 12 ? __builtin_bit_cast(uint32_t, flat[f_bm + i]) : (i == 12 ? __builtin_bit_cast(uint32_t, flat[f_bv]) : 0u); }
  packed[out] = word;
  if (flags) atomicOr(status, flags);
}

// packed = flat[0 .. nw) | mean (64) | istd (64) | clip: nw = the flat block without log_std
__global__ void __launch_bounds__(PREP_THREADS) k_pack_gnn(const float* __restrict__ flat, int nw, const double* __restrict__ st, float epsf, float clipf,
                                                           float* __restrict__ packed, int total, int32_t* status) {
  const int i = blockIdx.x * PREP_THREADS + threadIdx.x;
  if (i >= total) return;
  if (i < nw) {
    const float w = flat[i];
    packed[i] = w;
    const int flags = prep_flags(w);
    if (flags) atomicOr(status, flags);
  } else packed[i] = prep_scaler_word(st, 64, i - nw, epsf, clipf);
}

// ------------------------------------------------------------------------------------------------ batch statistics
// sums / a row of partial sums: S obs_c (C) | S obs_c^2 (C) | S ret | S ret^2 | S adv | S adv^2 [| B: sums only]
__global__ void __launch_bounds__(PREP_THREADS) k_prep_stats(const float* __restrict__ obs, const float* __restrict__ ret, const float* __restrict__ adv, int B, int C,
                                                             int rows_per_group, double* partials, unsigned int* counter, double* __restrict__ sums) {
  __shared__ double red[2048];      // 2 x RG x C doubles for the columns (16 x 64, 11 x 88), then 4 x 256 for the per-sample sums
  __shared__ int is_last;
  const int t = threadIdx.x, W = 2 * C + 4, G = gridDim.x;
  const long long r_lo = (long long)blockIdx.x * rows_per_group;
  const long long r_hi = r_lo + rows_per_group < B ? r_lo + rows_per_group : B;
  double* mine = partials + (size_t)blockIdx.x * W;
  // columns: thread t owns the 16-byte column group t % (C / 4) of the rows r_lo + t / (C / 4), + RG, ... (RG = 16 row groups for C = 64, 11
  // for C = 88), four loads in flight; a row group's order of additions is fixed by (r_lo, r_hi) alone
  const int CG = C >> 2, RG = PREP_THREADS / CG, cg = t % CG, rg = t / CG;
  double s[4] = {0.0, 0.0, 0.0, 0.0}, ss[4] = {0.0, 0.0, 0.0, 0.0};
  if (rg < RG) {
    const prep_f4* __restrict__ o4 = reinterpret_cast<const prep_f4*>(obs);
    long long r = r_lo + rg;
    for (; r + 3LL * RG < r_hi; r += 4LL * RG) {
      prep_f4 x[4];
#pragma unroll
      for (int u = 0; u < 4; u++) x[u] = o4[(r + (long long)u * RG) * CG + cg];
#pragma unroll
      for (int u = 0; u < 4; u++)
#pragma unroll
        for (int k = 0; k < 4; k++) { const double v = (double)x[u][k]; s[k] += v; ss[k] += v * v; }
    }
    for (; r < r_hi; r += RG) {
      const prep_f4 x = o4[r * CG + cg];
#pragma unroll
      for (int k = 0; k < 4; k++) { const double v = (double)x[k]; s[k] += v; ss[k] += v * v; }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) { red[2 * (rg * C + 4 * cg + k)] = s[k]; red[2 * (rg * C + 4 * cg + k) + 1] = ss[k]; }
  }
  __syncthreads();
  if (t < C) {
    double a = 0.0, b = 0.0;
    for (int k = 0; k < RG; k++) { a += red[2 * (k * C + t)]; b += red[2 * (k * C + t) + 1]; }
    mine[t] = a; mine[C + t] = b;
  }
  __syncthreads();
  // returns and advantages: thread t owns the rows r_lo + t, + 256, ...; then a halving tree
  double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
  for (long long r = r_lo + t; r < r_hi; r += PREP_THREADS) {
    const double x = (double)ret[r], y = (double)adv[r];
    q0 += x; q1 += x * x; q2 += y; q3 += y * y;
  }
  red[4 * t] = q0; red[4 * t + 1] = q1; red[4 * t + 2] = q2; red[4 * t + 3] = q3;
  __syncthreads();
  for (int w = PREP_THREADS / 2; w > 0; w >>= 1) {
    if (t < w)
      for (int k = 0; k < 4; k++) red[4 * t + k] += red[4 * (t + w) + k];
    __syncthreads();
  }
  if (t < 4) mine[2 * C + t] = red[t];
  // publish the row, take a ticket; the last workgroup to arrive adds the rows in row order
  __threadfence();
  __syncthreads();
  if (t == 0) is_last = atomicAdd(counter, 1u) == (unsigned int)(G - 1);
  __syncthreads();
  if (!is_last) return;
  __threadfence();
  if (t < W) {
    // device-scope loads (the rows were written by other workgroups), sixteen in flight; added in row order
    unsigned long long* col = reinterpret_cast<unsigned long long*>(partials) + t;
    double a = 0.0;
    int g = 0;
    for (; g + 16 <= G; g += 16) {
      unsigned long long u[16];
#pragma unroll
      for (int k = 0; k < 16; k++) u[k] = __hip_atomic_load(col + (size_t)(g + k) * W, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
      for (int k = 0; k < 16; k++) a += __builtin_bit_cast(double, u[k]);
    }
    for (; g < G; g++) a += __builtin_bit_cast(double, __hip_atomic_load(col + (size_t)g * W, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    sums[t] = a;
  }
  if (t == 0) { sums[W] = (double)B; *counter = 0u; }
}

// ------------------------------------------------------------------------------------------------ merge and apply
// RunningStandardScaler.update on one feature, operation for operation (train/ppo.py)
__device__ __forceinline__ void prep_merge(double s, double ss, double n, double count, double& mean, double& var) {
  const double bmean = s / n;
  double bvar = ss / n - bmean * bmean;
  bvar = bvar < 0.0 ? 0.0 : bvar;                       // clamp_min(0): a NaN stays a NaN
  double nm1 = n - 1.0; nm1 = nm1 < 1.0 ? 1.0 : nm1;
  bvar = bvar * n / nm1;
  const double delta = bmean - mean, tot = count + n;
  const double m2 = var * count + bvar * n + delta * delta * count * n / tot;
  mean = mean + delta * n / tot; var = m2 / tot;
}

__global__ void __launch_bounds__(128) k_prep_merge(const double* __restrict__ sums, int C, double* __restrict__ obs_state, double* __restrict__ val_state, int freeze_obs) {
  const int t = threadIdx.x;
  const double n = sums[2 * C + 4];
  if (t < C && !freeze_obs) {
    double mean = obs_state[t], var = obs_state[C + t];
    prep_merge(sums[t], sums[C + t], n, obs_state[2 * C], mean, var);
    obs_state[t] = mean; obs_state[C + t] = var;
  }
  if (t == 127) {
    double mean = val_state[0], var = val_state[1]; const double count = val_state[2];
    prep_merge(sums[2 * C], sums[2 * C + 1], n, count, mean, var);
    val_state[0] = mean; val_state[1] = var; val_state[2] = count + n;
  }
  __syncthreads();      // every thread has read the count before it moves
  if (t == 0 && !freeze_obs) obs_state[2 * C] = obs_state[2 * C] + n;
}

__device__ __forceinline__ float prep_norm(float x, double mean, double den, double clip) {
  double y = ((double)x - mean) / den;
  y = y < -clip ? -clip : (y > clip ? clip : y);      // clamp: a NaN stays a NaN
  return (float)y;
}

__global__ void __launch_bounds__(PREP_THREADS) k_prep_apply(const float* __restrict__ obs, const float* __restrict__ ret, const float* __restrict__ old_val,
                                                             const float* __restrict__ adv, int B, int C, int vec_groups, const double* __restrict__ sums,
                                                             const double* __restrict__ obs_state, const double* __restrict__ val_state, double eps, double clip,
                                                             float* __restrict__ obs_n, float* __restrict__ ret_n, float* __restrict__ old_val_n, float* __restrict__ adv_n) {
  __shared__ double s_mean[96], s_den[96];
  const int t = threadIdx.x;
  if ((int)blockIdx.x < vec_groups) {      // observations: one 16-byte vector per thread (C is a multiple of 4: a vector never crosses a row)
    if (t < C) { s_mean[t] = obs_state[t]; s_den[t] = sqrt(obs_state[C + t]) + eps; }
    __syncthreads();
    const long long v = (long long)blockIdx.x * PREP_THREADS + t, nvec = (long long)B * C / 4;
    if (v >= nvec) return;
    const unsigned CG = (unsigned)C >> 2, base = (unsigned)(((unsigned long long)blockIdx.x * PREP_THREADS) % CG);      // uniform: scalar arithmetic
    const int c0 = 4 * (int)((base + (unsigned)t) % CG);      // the vector's first column
    const prep_f4 x = reinterpret_cast<const prep_f4*>(obs)[v];
    prep_f4 y;
#pragma unroll
    for (int k = 0; k < 4; k++) y[k] = prep_norm(x[k], s_mean[c0 + k], s_den[c0 + k], clip);
    reinterpret_cast<prep_f4*>(obs_n)[v] = y;
    return;
  }
  // returns, old values, advantages: one sample per thread
  const long long r = (long long)((int)blockIdx.x - vec_groups) * PREP_THREADS + t;
  if (r >= B) return;
  const double vmean = val_state[0], vden = sqrt(val_state[1]) + eps;
  const double n = sums[2 * C + 4], sa = sums[2 * C + 2], saa = sums[2 * C + 3];
  const double amean = sa / n;
  double avar = (saa - sa * sa / n) / (n - 1.0);      // the unbiased variance from the sums
  avar = avar < 0.0 ? 0.0 : avar;
  const double aden = sqrt(avar) + 1e-8;
  ret_n[r] = prep_norm(ret[r], vmean, vden, clip);
  old_val_n[r] = prep_norm(old_val[r], vmean, vden, clip);
  adv_n[r] = (float)(((double)adv[r] - amean) / aden);
}

// ------------------------------------------------------------------------------------------------ entry points
static int prep_on_current_device(const void* p) {
  hipPointerAttribute_t at; int dev = -1;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return 0; }
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  return at.type == hipMemoryTypeDevice && at.device == dev;
}

static int prep_stats_groups(int B) {
  int g = (B + PREP_MIN_ROWS - 1) / PREP_MIN_ROWS;
  return g > PREP_MAX_GROUPS ? PREP_MAX_GROUPS : g;
}

static int prep_pack_check(const char* who, const float* flat, const double* st, double eps, double clip, const float* packed, const int32_t* status, char* msg, size_t len) {
  const char* why = nullptr;
  if (!flat || !packed || !status) why = "null argument";
  else if (!(eps >= 0.0) || !(clip > 0.0)) why = "eps must be >= 0 and clip > 0";
  else if (reinterpret_cast<uintptr_t>(packed) & 15) why = "packed must be 16-byte aligned (the forward kernels read it with 16-byte loads)";
  else if ((reinterpret_cast<uintptr_t>(flat) | reinterpret_cast<uintptr_t>(status)) & 3) why = "flat and status must be 4-byte aligned";
  else if (st && (reinterpret_cast<uintptr_t>(st) & 7)) why = "the scaler state must be 8-byte aligned";
  else if (!prep_on_current_device(flat) || !prep_on_current_device(packed) || !prep_on_current_device(status) || (st && !prep_on_current_device(st)))
    why = "the buffers are not device memory of the calling thread's current device";
  if (!why) return 0;
  snprintf(msg, len, "%s: %s", who, why);
  return -1;
}

extern "C" {

int lm_mlp_pack_params(const float* flat, int num_obs, const double* scaler_state, double eps, double clip, float* packed, int32_t* status, void* stream) {
  char msg[192];
  if (num_obs != 64 && num_obs != 88) return lm_internal_fail(LM_EINVAL, "lm_mlp_pack_params: num_obs must be 64 or 88");
  if (prep_pack_check("lm_mlp_pack_params", flat, scaler_state, eps, clip, packed, status, msg, sizeof msg)) return lm_internal_fail(LM_EINVAL, msg);
  const int kpad = (num_obs + 31) & ~31;
  const int total = 2 * num_obs + 4 + 256 * kpad + 256 + 128 * 256 + 128 + 64 * 128 + 64 + 16 * 64 + 16;
  if (total != lm_mlp_param_count_obs(num_obs)) return lm_internal_fail(-2, "lm_mlp_pack_params: the packed layout and lm_mlp_param_count_obs disagree");
  hipLaunchKernelGGL(k_pack_mlp, dim3((total + PREP_THREADS - 1) / PREP_THREADS), dim3(PREP_THREADS), 0, (hipStream_t)stream, flat, num_obs, scaler_state, (float)eps,
                     (float)clip, reinterpret_cast<uint32_t*>(packed), total, status);
  return hipGetLastError() == hipSuccess ? 0 : lm_internal_fail(-2, "lm_mlp_pack_params: launch failed");
}

int lm_gnn_pack_params(const float* flat, int num_obs, const double* scaler_state, double eps, double clip, float* packed, int32_t* status, void* stream) {
  char msg[192];
  if (num_obs != 64) return lm_internal_fail(LM_EINVAL, "lm_gnn_pack_params: num_obs must be 64 (the GNN reads the 64-wide observation layout)");
  if (prep_pack_check("lm_gnn_pack_params", flat, scaler_state, eps, clip, packed, status, msg, sizeof msg)) return lm_internal_fail(LM_EINVAL, msg);
  const int nw = lm_gnn_grad_param_count() - 12, total = nw + 2 * 64 + 1;
  if (total != lm_gnn_param_count()) return lm_internal_fail(-2, "lm_gnn_pack_params: the packed layout and lm_gnn_param_count disagree");
  hipLaunchKernelGGL(k_pack_gnn, dim3((total + PREP_THREADS - 1) / PREP_THREADS), dim3(PREP_THREADS), 0, (hipStream_t)stream, flat, nw, scaler_state, (float)eps, (float)clip,
                     packed, total, status);
  return hipGetLastError() == hipSuccess ? 0 : lm_internal_fail(-2, "lm_gnn_pack_params: launch failed");
}

int lm_ppo_batch_sums_len(int C) { return (C == 64 || C == 88) ? 2 * C + 5 : LM_EINVAL; }

long long lm_ppo_batch_stats_workspace(int B, int C) {
  if (C != 64 && C != 88) return lm_internal_fail(LM_EINVAL, "lm_ppo_batch_stats_workspace: C must be 64 or 88");
  if (B < 2) return lm_internal_fail(LM_EINVAL, "lm_ppo_batch_stats_workspace: B must be >= 2 (the unbiased deviation of one sample is not a number)");
  return PREP_WS_HEADER + (long long)prep_stats_groups(B) * (2 * C + 4) * (long long)sizeof(double);
}

int lm_ppo_batch_stats(const float* obs, const float* ret, const float* adv, int B, int C, double* sums, void* workspace, long long workspace_bytes, void* stream) {
  if (!obs || !ret || !adv || !sums || !workspace) return lm_internal_fail(LM_EINVAL, "lm_ppo_batch_stats: null argument");
  if (C != 64 && C != 88) return lm_internal_fail(LM_EINVAL, "lm_ppo_batch_stats: C must be 64 or 88");
  if (B < 2) return lm_internal_fail(LM_EINVAL, "lm_ppo_batch_stats: B must be >= 2 (the unbiased deviation of one sample is not a number)");
  if (reinterpret_cast<uintptr_t>(obs) & 15) return lm_internal_fail(LM_EINVAL, "lm_ppo_batch_stats: obs must be 16-byte aligned (16-byte loads)");
  if ((reinterpret_cast<uintptr_t>(ret) | reinterpret_cast<uintptr_t>(adv)) & 3) return lm_internal_fail(LM_EINVAL, "lm_ppo_batch_stats: ret and adv must be 4-byte aligned");
  if ((reinterpret_cast<uintptr_t>(sums) & 7) || (reinterpret_cast<uintptr_t>(workspace) & 15))
    return lm_internal_fail(LM_EINVAL, "lm_ppo_batch_stats: sums must be 8-byte and the workspace 16-byte aligned");
  if (workspace_bytes < lm_ppo_batch_stats_workspace(B, C)) return lm_internal_fail(LM_EINVAL, "lm_ppo_batch_stats: the workspace is too small (lm_ppo_batch_stats_workspace)");
  if (!prep_on_current_device(obs) || !prep_on_current_device(ret) || !prep_on_current_device(adv) || !prep_on_current_device(sums) || !prep_on_current_device(workspace))
    return lm_internal_fail(LM_EINVAL, "lm_ppo_batch_stats: the buffers are not device memory of the calling thread's current device");
  const int G = prep_stats_groups(B), rows = (B + G - 1) / G;
  const int launched = (B + rows - 1) / rows;      // <= G: no workgroup without a row
  hipLaunchKernelGGL(k_prep_stats, dim3(launched), dim3(PREP_THREADS), 0, (hipStream_t)stream, obs, ret, adv, B, C, rows,
                     reinterpret_cast<double*>(static_cast<char*>(workspace) + PREP_WS_HEADER), static_cast<unsigned int*>(workspace), sums);
  return hipGetLastError() == hipSuccess ? 0 : lm_internal_fail(-2, "lm_ppo_batch_stats: launch failed");
}

int lm_ppo_batch_apply(const float* obs, const float* ret, const float* old_val, const float* adv, int B, int C, const double* sums, double* obs_state,
                       double* val_state, int freeze_obs, double eps, double clip, float* obs_n, float* ret_n, float* old_val_n, float* adv_n, void* stream) {
  if (!obs || !ret || !old_val || !adv || !sums || !obs_state || !val_state || !obs_n || !ret_n || !old_val_n || !adv_n)
    return lm_internal_fail(LM_EINVAL, "lm_ppo_batch_apply: null argument");
  if (C != 64 && C != 88) return lm_internal_fail(LM_EINVAL, "lm_ppo_batch_apply: C must be 64 or 88");
  if (B < 2) return lm_internal_fail(LM_EINVAL, "lm_ppo_batch_apply: B must be >= 2 (the unbiased deviation of one sample is not a number)");
  if (!(eps >= 0.0) || !(clip > 0.0)) return lm_internal_fail(LM_EINVAL, "lm_ppo_batch_apply: eps must be >= 0 and clip > 0");
  if ((reinterpret_cast<uintptr_t>(obs) | reinterpret_cast<uintptr_t>(obs_n)) & 15)
    return lm_internal_fail(LM_EINVAL, "lm_ppo_batch_apply: obs and obs_n must be 16-byte aligned (16-byte loads and stores)");
  if ((reinterpret_cast<uintptr_t>(ret) | reinterpret_cast<uintptr_t>(old_val) | reinterpret_cast<uintptr_t>(adv) | reinterpret_cast<uintptr_t>(ret_n) |
       reinterpret_cast<uintptr_t>(old_val_n) | reinterpret_cast<uintptr_t>(adv_n)) & 3)
    return lm_internal_fail(LM_EINVAL, "lm_ppo_batch_apply: the per-sample blocks must be 4-byte aligned");
  if ((reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(obs_state) | reinterpret_cast<uintptr_t>(val_state)) & 7)
    return lm_internal_fail(LM_EINVAL, "lm_ppo_batch_apply: sums and the scaler states must be 8-byte aligned");
  const void* all[] = {obs, ret, old_val, adv, sums, obs_state, val_state, obs_n, ret_n, old_val_n, adv_n};
  for (const void* p : all)
    if (!prep_on_current_device(p)) return lm_internal_fail(LM_EINVAL, "lm_ppo_batch_apply: the buffers are not device memory of the calling thread's current device");
  const long long nvec = (long long)B * C / 4;
  const long long vec_groups = (nvec + PREP_THREADS - 1) / PREP_THREADS, row_groups = ((long long)B + PREP_THREADS - 1) / PREP_THREADS;
  if (vec_groups + row_groups > 0x7fffffffLL) return lm_internal_fail(LM_EINVAL, "lm_ppo_batch_apply: B x C is beyond one launch");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_prep_merge, dim3(1), dim3(128), 0, s, sums, C, obs_state, val_state, freeze_obs);
  if (hipGetLastError() != hipSuccess) return lm_internal_fail(-2, "lm_ppo_batch_apply: launching the merge kernel failed");
  hipLaunchKernelGGL(k_prep_apply, dim3((unsigned)(vec_groups + row_groups)), dim3(PREP_THREADS), 0, s, obs, ret, old_val, adv, B, C, (int)vec_groups, sums,
                     (const double*)obs_state, (const double*)val_state, eps, clip, obs_n, ret_n, old_val_n, adv_n);
  return hipGetLastError() == hipSuccess ? 0 : lm_internal_fail(-2, "lm_ppo_batch_apply: launching the apply kernel failed");
}

}  // extern "C"
