// Third translation unit of liblm_engine.so: the evaluation builds of the two persistent rollout kernels (k_rollout_ev, k_rollout_mlp_ev; template
// flag EV): LM_EV_DET = the policy tile's mean-action epilogue (lm_rollout_set_deterministic), LM_EV_REC = the episode record
// (lm_rollout_set_episode_record).  Kernels of their own, as the *_cf step kernels are - a plan with both switches off launches k_rollout /
// k_rollout_mlp - and a unit of their own, as k_step_w2 is: with these instantiations in lm_engine.hip the compiler laid k_rollout_mlp out differently,
// although its source had not changed.  The device body is the one of lm_rollout_dev.h, shared with lm_engine_tr.hip; this unit
// holds the kernels that instantiate it and their launcher.
// Instantiated: LM_EV_DET for every policy / width; LM_EV_REC only where it builds without scratch memory, the resident MLP tile on 64-wide
// observations (lm_internal_rollout_records).
#undef LM_STAMPS              // diagnostic switches of the whole-library builds do not apply to this unit (their device globals live in lm_engine.hip)
#undef LM_COUNT_PASS2
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lm_math.h"
#include "lm_rng.h"
#include "../../include/lm_engine.h"
#include "../../include/lm_policy.h"
#include "lm_policy_dev.h"
#include "lm_step.h"
#include "lm_rollout_dev.h"

template <int NOBS, int POLICY, int EV>
__global__ void __launch_bounds__(256) k_rollout_ev(StepArgs A, RolloutDev R, RolloutEv) { rollout_block_ev<NOBS, POLICY, EV>(A, R); }
template <int NOBS, int EV>
__global__ void __launch_bounds__(256) k_rollout_mlp_ev(StepArgs A, RolloutDev R, RolloutEv E) { rollout_mlp_block_ev<NOBS, EV>(A, R, E, RolloutTraj{}); }

extern "C" __attribute__((visibility("hidden"))) int lm_internal_launch_rollout_ev(const StepArgs* A, const RolloutDev* D, const RolloutEv* E, int ev, int policy, int nobs,
                                                                                  int nblocks, hipStream_t s) {
  void (*kern)(StepArgs, RolloutDev, RolloutEv) = nullptr;
  if (policy == LM_POLICY_MLP && nobs == 64) kern = ev == LM_EV_DET ? k_rollout_mlp_ev<64, LM_EV_DET> : ev == LM_EV_REC ? k_rollout_mlp_ev<64, LM_EV_REC> : k_rollout_mlp_ev<64, LM_EV_DET | LM_EV_REC>;
  else if (policy == LM_POLICY_MLP && nobs == LM_MAX_OBS && ev == LM_EV_DET) kern = k_rollout_mlp_ev<LM_MAX_OBS, LM_EV_DET>;
  else if (policy == LM_POLICY_GNN && nobs == 64 && ev == LM_EV_DET) kern = k_rollout_ev<64, LM_POLICY_GNN, LM_EV_DET>;
  else return -1;
  hipLaunchKernelGGL(kern, dim3(nblocks), dim3(256), 0, s, *A, *D, *E);
  return 0;
}
