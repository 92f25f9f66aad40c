// Fourth rollout translation unit of liblm_engine.so: the builds of the persistent MLP rollout kernel that keep a TRAJECTORY record
// (lm_rollout_set_trajectory_record, include/lm_policy.h): k_rollout_mlp_tr<64, EV> with LM_EV_TRAJ in EV, alone or with LM_EV_DET and / or
// LM_EV_REC of lm_engine_ev.hip.  Kernels of their own and a unit of their own, for the reason lm_engine_ev.hip is one: another instantiation
// in a unit moves the code of its neighbours.  The device body is the one of lm_rollout_dev.h, shared with lm_engine_ev.hip;
// this unit holds the kernels that instantiate it with the third flag and their launcher.  The record's arguments travel in RolloutTraj, next to
// RolloutEv.
// Instantiated: the resident MLP tile on 64-wide observations only, and only the combinations that build with 0 bytes of scratch memory
// (lm_internal_rollout_tr_built; the figures are in DESIGN.md 5.3.1).  Every other plan with a trajectory record attached takes the graph.
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

template <int NOBS, int EV>
__global__ void __launch_bounds__(256) k_rollout_mlp_tr(StepArgs A, RolloutDev R, RolloutEv E, RolloutTraj TJ) { rollout_mlp_block_ev<NOBS, EV>(A, R, E, TJ); }

// which combinations are built: LM_TR_BUILDS is a bit mask over the DET | REC bits that accompany LM_EV_TRAJ (bit 0: TRAJ alone, bit 1: TRAJ | DET,
// bit 2: TRAJ | REC, bit 3: TRAJ | DET | REC); a combination is listed only if it compiles with 0 bytes of scratch memory
#ifndef LM_TR_BUILDS
#define LM_TR_BUILDS 0xF
#endif
extern "C" __attribute__((visibility("hidden"))) int lm_internal_rollout_tr_built(int ev, int policy, int nobs) {
  return (ev & LM_EV_TRAJ) && policy == LM_POLICY_MLP && nobs == 64 && ((LM_TR_BUILDS >> (ev & (LM_EV_DET | LM_EV_REC))) & 1);
}
extern "C" __attribute__((visibility("hidden"))) int lm_internal_launch_rollout_tr(const StepArgs* A, const RolloutDev* D, const RolloutEv* E, const RolloutTraj* TJ, int ev,
                                                                                  int policy, int nobs, int nblocks, hipStream_t s) {
  if (!lm_internal_rollout_tr_built(ev, policy, nobs)) return -1;
  void (*kern)(StepArgs, RolloutDev, RolloutEv, RolloutTraj) = nullptr;
  switch (ev & (LM_EV_DET | LM_EV_REC)) {
#if LM_TR_BUILDS & 1
    case 0: kern = k_rollout_mlp_tr<64, LM_EV_TRAJ>; break;
#endif
#if LM_TR_BUILDS & 2
    case LM_EV_DET: kern = k_rollout_mlp_tr<64, LM_EV_TRAJ | LM_EV_DET>; break;
#endif
#if LM_TR_BUILDS & 4
    case LM_EV_REC: kern = k_rollout_mlp_tr<64, LM_EV_TRAJ | LM_EV_REC>; break;
#endif
#if LM_TR_BUILDS & 8
    case LM_EV_DET | LM_EV_REC: kern = k_rollout_mlp_tr<64, LM_EV_TRAJ | LM_EV_DET | LM_EV_REC>; break;
#endif
    default: return -1;
  }
  hipLaunchKernelGGL(kern, dim3(nblocks), dim3(256), 0, s, *A, *D, *E, *TJ);
  return 0;
}
