// Second translation unit of liblm_engine.so: the step compiled for two wavefronts per SIMD (k_step_w2) and its launcher.  LM_WAVES2 gives the
// step's device headers the layout that fits (<= 256 registers, <= 20 KB of LDS per wavefront; see the comment at STASH_SLOTS in lm_dynamics.h);
// lm_step dispatches the kernel beyond 32 768 envs on locomotion engines (+ 5-8 % from 36 864 envs, + 9 % at 65 536, + 14 % at
// 131 072, + 18 % at 262 144; slower below 24 576).  A separate unit so that the one-wavefront kernels of lm_engine.hip keep their register
// allocation and code layout.
#ifndef LM_WAVES2
#define LM_WAVES2 1
#endif
#undef LM_STAMPS              // diagnostic switches of the whole-library builds do not apply to this unit (their device globals live in lm_engine.hip)
#undef LM_COUNT_PASS2
#include "lm_step.h"

__global__ void __launch_bounds__(64) LM_STEP_ATTR k_step_w2(StepArgs A) {
  LM_STEP_SMEM(64)
  LM_STEP_PROLOGUE
  // locomotion only: the plate specialisation does not live in 256 registers (measured with both in this kernel: 300 against 533 M env-steps/s on
  // the manipulation task at 65 536 envs), so manipulation and co-training engines stay on the one-wavefront kernel at every size
  // last argument 0: both passes of a sub-step read the stash (lm_dynamics.h): in 256 registers the first pass on registers costs 40 B more scratch
  step_body<0, 0, 0, 0, 0, 0>(A, P, sTab, sObs, sSt, sStash);
  LM_STEP_EPILOGUE
}
extern "C" __attribute__((visibility("hidden"))) void lm_internal_launch_step_w2(const StepArgs* A, int nblocks, hipStream_t s) {
  hipLaunchKernelGGL(k_step_w2, dim3(nblocks), dim3(64), 0, s, *A);
}
