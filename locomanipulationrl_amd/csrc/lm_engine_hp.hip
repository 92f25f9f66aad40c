// Translation unit of liblm_engine.so: the randomised step kernels of an engine whose caller holds per-env physics parameters
// (lm_enable_env_params): k_step_dr_hp and k_step_dr_pd_hp are k_step_dr / k_step_dr_pd with step_body's template switch HP on.
// In them the value of every held row of the hold table (StepArgs::env_params, mask StepArgs::env_mask) replaces what the channel of that row
// produced, after the channels have drawn and before the record rows are written.  Kernels of their own, as the *_cf kernels are, so that an
// engine that did not opt in launches exactly what it launched before; a unit of their own, as k_step_w2 is, so that the kernels of
// lm_engine.hip keep their register allocation and code layout.  lm_step dispatches here while env params are enabled.
#undef LM_STAMPS              // diagnostic switches of the whole-library builds do not apply to this unit (their device globals live in lm_engine.hip)
#undef LM_COUNT_PASS2
#undef LM_WAVES2
#undef LM_PASS0_STASH
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lm_math.h"
#include "lm_rng.h"
#include "../../include/lm_engine.h"
#include "../../include/lm_policy.h"
#include "lm_step.h"

__global__ void __launch_bounds__(64) k_step_dr_hp(StepArgs A) {              // velocity-drive tasks (kinds 0, 1)
  LM_STEP_SMEM(64)
  if (kind == 0) step_body<0, 0, 1, 0, 0, 1, 0, 0, 1>(A, P, sTab, sObs, sSt, sStash); else step_body<1, 0, 1, 0, 0, 1, 0, 0, 1>(A, P, sTab, sObs, sSt, sStash);
}

__global__ void __launch_bounds__(64) k_step_dr_pd_hp(StepArgs A) {           // PD-actuator families (kinds 2 ... 5)
  LM_STEP_SMEM(LM_MAX_OBS)
  if (kind == 2) step_body<0, 1, 1, 0, 0, 1, 0, 0, 1>(A, P, sTab, sObs, sSt, sStash); else if (kind == 3) step_body<1, 1, 1, 0, 0, 1, 0, 0, 1>(A, P, sTab, sObs, sSt, sStash);
  else if (kind == 4) step_body<0, 2, 1, 0, 0, 1, 0, 0, 1>(A, P, sTab, sObs, sSt, sStash); else step_body<1, 2, 1, 0, 0, 1, 0, 0, 1>(A, P, sTab, sObs, sSt, sStash);
}

extern "C" __attribute__((visibility("hidden"))) void lm_internal_launch_step_hp(const StepArgs* A, int pd, int nblocks, hipStream_t s) {
  hipLaunchKernelGGL(pd ? k_step_dr_pd_hp : k_step_dr_hp, dim3(nblocks), dim3(64), 0, s, *A);
}
