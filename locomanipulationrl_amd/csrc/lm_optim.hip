// lm_optim.hip -- the optimiser step of the PPO update on the device (include/lm_policy.h): lm_adam_clip_step = torch.nn.utils.clip_grad_norm_
// followed by torch.optim.Adam (no weight decay, no amsgrad) on one flat fp32 block, lm_kl_adaptive_lr = the KL-adaptive rate of
// train/ppo.py PPO.update, and the state block (double [LM_OPTIM_STATE]) the two share: the rate and the step count live on the device, so
// the epoch loop never waits for the host.
//
// Launch form of lm_adam_clip_step, and why it cannot race: TWO launches on one stream.
//   k_optim_norm   ONE workgroup.  Reads grad and state[lr, step]; writes state[step, grad_norm, clip_coef, step_size, bc2_sqrt].
//   k_optim_step   many workgroups.  Reads grad and state[clip_coef, step_size, bc2_sqrt]; writes params, exp_avg, exp_avg_sq.  Writes no slot
//                  of state.
// Every slot of state that a launch writes is read only by the workgroup that writes it (k_optim_norm has one) or by a later launch, and the
// stream orders the launches: a workgroup of k_optim_step that starts late sees what every other one sees, because nothing it reads is
// written while it runs.  One launch in which the first workgroup published the step count to the others would need them to agree on
// whether they run before or after the store; this form has no such question.  lm_kl_adaptive_lr is one workgroup of its own and the only
// writer of state[lr] besides lm_optim_state_init.
// Determinism: no atomics.  The squared norm is summed in double: thread t of 1024 takes the 16-byte vectors t, t + 1024, ... (two chains),
// the n % 4 tail goes to threads 0..2, then a halving tree in LDS - an order fixed by n alone.
// Arithmetic per element: in double on the vector ALU (the product flags make fp32 division and square root 1-ulp approximations; the double
// sequences are correctly rounded), one rounding to fp32 per stored value.  At most 64 793 elements: the cost does not show.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/lm_policy.h"
#include "../../include/lm_engine.h"
#include "lm_internal.h"

typedef float opt_f4 __attribute__((ext_vector_type(4)));

#define OPT_NORM_THREADS 1024
#define OPT_STEP_THREADS 64      // one wavefront of 16-byte lanes per workgroup: 64 793 elements spread over 254 compute units

// slots 0..4 are the interface (include/lm_policy.h); 5 and 6 carry what k_optim_norm derives once for k_optim_step
enum { OPT_STEP_SIZE = 5, OPT_BC2_SQRT = 6 };

__global__ void __launch_bounds__(OPT_NORM_THREADS) k_optim_norm(const float* __restrict__ grad, int n, double* __restrict__ state, double beta1,
                                                                 double beta2, double max_norm) {
  __shared__ double red[OPT_NORM_THREADS];
  const int t = threadIdx.x, n4 = n >> 2;
  const opt_f4* __restrict__ g4 = reinterpret_cast<const opt_f4*>(grad);
  double s0 = 0.0, s1 = 0.0;
  for (int i = t; i < n4; i += OPT_NORM_THREADS) {
    const opt_f4 x = g4[i];
    s0 += (double)x.x * (double)x.x + (double)x.y * (double)x.y;
    s1 += (double)x.z * (double)x.z + (double)x.w * (double)x.w;
  }
  if (t < (n & 3)) { const double x = (double)grad[4 * n4 + t]; s0 += x * x; }
  red[t] = s0 + s1;
  __syncthreads();
  for (int w = OPT_NORM_THREADS / 2; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  if (t == 0) {
    const double norm = sqrt(red[0]);
    double coef = max_norm / (norm + 1e-6);
    coef = coef > 1.0 ? 1.0 : coef;                       // clamp(max = 1): a NaN stays a NaN, as in torch
    const double step = state[LM_OPTIM_STEP] + 1.0;
    state[LM_OPTIM_STEP] = step; state[LM_OPTIM_GRAD_NORM] = norm; state[LM_OPTIM_CLIP_COEF] = coef;
    state[OPT_STEP_SIZE] = state[LM_OPTIM_LR] / (1.0 - pow(beta1, step));
    state[OPT_BC2_SQRT] = sqrt(1.0 - pow(beta2, step));
  }
}

struct OptStep { double coef, beta1, beta2, eps, step_size, bc2_sqrt; int c_lo, c_hi; float c_min; };

__device__ __forceinline__ void opt_elem(const OptStep& S, int e, float& p, float g, float& m, float& v) {
  const double gd = S.coef * (double)g;
  const double md = S.beta1 * (double)m + (1.0 - S.beta1) * gd;
  const double vd = S.beta2 * (double)v + (1.0 - S.beta2) * gd * gd;
  m = (float)md; v = (float)vd;
  float q = (float)((double)p - S.step_size * md / (sqrt(vd) / S.bc2_sqrt + S.eps));
  if (e >= S.c_lo && e < S.c_hi) q = q < S.c_min ? S.c_min : q;      // the floor after the step (a NaN stays a NaN)
  p = q;
}

__global__ void __launch_bounds__(OPT_STEP_THREADS) k_optim_step(float* __restrict__ params, const float* __restrict__ grad, float* __restrict__ exp_avg,
                                                                 float* __restrict__ exp_avg_sq, int n, const double* __restrict__ state, lm_optim_hyper hp) {
  const int idx = blockIdx.x * OPT_STEP_THREADS + threadIdx.x, n4 = n >> 2;
  OptStep S;
  S.coef = state[LM_OPTIM_CLIP_COEF]; S.step_size = state[OPT_STEP_SIZE]; S.bc2_sqrt = state[OPT_BC2_SQRT];
  S.beta1 = hp.beta1; S.beta2 = hp.beta2; S.eps = hp.eps;
  S.c_lo = hp.clamp_offset; S.c_hi = hp.clamp_offset + hp.clamp_count; S.c_min = hp.clamp_min;      // clamp_count 0: an empty range
  if (idx < n4) {      // 16-byte path: vector idx covers elements 4 idx .. 4 idx + 3 < n
    opt_f4 p = reinterpret_cast<opt_f4*>(params)[idx], m = reinterpret_cast<opt_f4*>(exp_avg)[idx], v = reinterpret_cast<opt_f4*>(exp_avg_sq)[idx];
    const opt_f4 g = reinterpret_cast<const opt_f4*>(grad)[idx];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      float pk = p[k], mk = m[k], vk = v[k];
      opt_elem(S, 4 * idx + k, pk, g[k], mk, vk);
      p[k] = pk; m[k] = mk; v[k] = vk;
    }
    reinterpret_cast<opt_f4*>(params)[idx] = p; reinterpret_cast<opt_f4*>(exp_avg)[idx] = m; reinterpret_cast<opt_f4*>(exp_avg_sq)[idx] = v;
  } else if (idx < n4 + (n & 3)) {      // scalar tail: elements 4 n4 .. n - 1
    const int e = 4 * n4 + (idx - n4);
    float p = params[e], m = exp_avg[e], v = exp_avg_sq[e];
    opt_elem(S, e, p, grad[e], m, v);
    params[e] = p; exp_avg[e] = m; exp_avg_sq[e] = v;
  }
}

// mean of `count` fp32 KL values in double, in index order, then the rule of PPO.update on doubles
__global__ void __launch_bounds__(64) k_optim_kl_lr(double* __restrict__ state, const float* __restrict__ kl, int count, double thr, double lr_min, double lr_max) {
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int i = 0; i < count; i++) s += (double)kl[i];
  const double mean = s / (double)count;
  double lr = state[LM_OPTIM_LR];
  if (thr > 0.0) {
    if (mean > thr * 2.0) { const double d = lr / 1.5; lr = d > lr_min ? d : lr_min; }
    else if (mean < thr / 2.0) { const double u = lr * 1.5; lr = u < lr_max ? u : lr_max; }
  }
  state[LM_OPTIM_KL] = mean; state[LM_OPTIM_LR] = lr;
}

__global__ void __launch_bounds__(64) k_optim_state_init(double* __restrict__ state, double lr, double step) {
  const int t = threadIdx.x;
  if (t >= LM_OPTIM_STATE) return;
  state[t] = t == LM_OPTIM_LR ? lr : (t == LM_OPTIM_STEP ? step : (t == LM_OPTIM_CLIP_COEF ? 1.0 : 0.0));
}

static int optim_on_current_device(const void* p) {
  hipPointerAttribute_t at; int dev = -1;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return 0; }
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  return at.type == hipMemoryTypeDevice && at.device == dev;
}

extern "C" {

int lm_optim_state_len(void) { return LM_OPTIM_STATE; }

int lm_optim_state_init(double* state, double lr, double step, void* stream) {
  if (!state) return lm_internal_fail(LM_EINVAL, "lm_optim_state_init: null state");
  if (!(step >= 0.0)) return lm_internal_fail(LM_EINVAL, "lm_optim_state_init: the step count must be >= 0");
  if (!optim_on_current_device(state)) return lm_internal_fail(LM_EINVAL, "lm_optim_state_init: state is not device memory of the calling thread's current device");
  hipLaunchKernelGGL(k_optim_state_init, dim3(1), dim3(64), 0, (hipStream_t)stream, state, lr, step);
  return hipGetLastError() == hipSuccess ? 0 : lm_internal_fail(-2, "lm_optim_state_init: launch failed");
}

int lm_adam_clip_step(float* params, const float* grad, float* exp_avg, float* exp_avg_sq, int n, double* state, const lm_optim_hyper* hyper,
                      void* stream) {
  if (!params || !grad || !exp_avg || !exp_avg_sq || !state || !hyper) return lm_internal_fail(LM_EINVAL, "lm_adam_clip_step: null argument");
  if (n < 1) return lm_internal_fail(LM_EINVAL, "lm_adam_clip_step: n must be >= 1");
  if (hyper->clamp_count < 0 || (hyper->clamp_count > 0 && (hyper->clamp_offset < 0 || hyper->clamp_offset >= n || hyper->clamp_count > n - hyper->clamp_offset)))
    return lm_internal_fail(LM_EINVAL, "lm_adam_clip_step: the clamp range must lie inside [0, n)");
  if ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(exp_avg) | reinterpret_cast<uintptr_t>(exp_avg_sq)) & 15)
    return lm_internal_fail(LM_EINVAL, "lm_adam_clip_step: params, grad and both moment blocks must be 16-byte aligned (16-byte loads and stores)");
  if (reinterpret_cast<uintptr_t>(state) & 7) return lm_internal_fail(LM_EINVAL, "lm_adam_clip_step: state must be 8-byte aligned");
  if (!optim_on_current_device(params) || !optim_on_current_device(grad) || !optim_on_current_device(exp_avg) || !optim_on_current_device(exp_avg_sq) ||
      !optim_on_current_device(state))
    return lm_internal_fail(LM_EINVAL, "lm_adam_clip_step: the buffers are not device memory of the calling thread's current device");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_optim_norm, dim3(1), dim3(OPT_NORM_THREADS), 0, s, grad, n, state, hyper->beta1, hyper->beta2, hyper->max_norm);
  if (hipGetLastError() != hipSuccess) return lm_internal_fail(-2, "lm_adam_clip_step: launching the norm kernel failed");
  const int work = (n >> 2) + (n & 3);
  hipLaunchKernelGGL(k_optim_step, dim3((work + OPT_STEP_THREADS - 1) / OPT_STEP_THREADS), dim3(OPT_STEP_THREADS), 0, s, params, grad, exp_avg, exp_avg_sq, n,
                     (const double*)state, *hyper);
  return hipGetLastError() == hipSuccess ? 0 : lm_internal_fail(-2, "lm_adam_clip_step: launching the step kernel failed");
}

int lm_kl_adaptive_lr(double* state, const float* kl, int count, double threshold, double lr_min, double lr_max, void* stream) {
  if (!state || !kl) return lm_internal_fail(LM_EINVAL, "lm_kl_adaptive_lr: null argument");
  if (count < 1) return lm_internal_fail(LM_EINVAL, "lm_kl_adaptive_lr: count must be >= 1");
  if (reinterpret_cast<uintptr_t>(state) & 7) return lm_internal_fail(LM_EINVAL, "lm_kl_adaptive_lr: state must be 8-byte aligned");
  if (!optim_on_current_device(state) || !optim_on_current_device(kl))
    return lm_internal_fail(LM_EINVAL, "lm_kl_adaptive_lr: the buffers are not device memory of the calling thread's current device");
  hipLaunchKernelGGL(k_optim_kl_lr, dim3(1), dim3(64), 0, (hipStream_t)stream, state, kl, count, threshold, lr_min, lr_max);
  return hipGetLastError() == hipSuccess ? 0 : lm_internal_fail(-2, "lm_kl_adaptive_lr: launch failed");
}

}  // extern "C"
