// lm_rollout_dev.h -- what the persistent rollout kernels of lm_engine.hip (k_rollout, k_rollout_mlp) and their evaluation builds in
// lm_engine_ev.hip share: the device-side argument block, the step as the stepping wavefront calls it, the policy tile's LDS.
#pragma once
#include "../../include/lm_policy.h"
#include "lm_policy_dev.h"
#include "lm_step.h"

struct RolloutDev {
  const float* params; const float* log_std;
  float *obs, *actions, *logp, *values, *rewards; int64_t* dones;
  long long* acc_steps; int T; uint32_t noise_seed;
};

// the step of the persistent kernel as a real call: its ~350 registers are then allocated separately from the policy tile's
// (last template argument 0: both passes of a sub-step read the stash, lm_dynamics.h - on registers the first pass costs these kernels, which sit at
// 512 registers, 130-190 B more scratch)
LM_DEV void step_dispatch(const StepArgs& B, const lm_params* P, float* sTab, float* sObs, float* sSt, float4* sStash) {
  if (P->variant == 0) { if (P->mode == LM_MODE_LOCO) step_body<0, 0, 0, 1, 0, 0>(B, P, sTab, sObs, sSt, sStash); else step_body<1, 0, 0, 1, 0, 0>(B, P, sTab, sObs, sSt, sStash); }
  else if (P->variant == 1) { if (P->mode == LM_MODE_LOCO) step_body<0, 1, 0, 1, 0, 0>(B, P, sTab, sObs, sSt, sStash); else step_body<1, 1, 0, 1, 0, 0>(B, P, sTab, sObs, sSt, sStash); }
  else { if (P->mode == LM_MODE_LOCO) step_body<0, 2, 0, 1, 0, 0>(B, P, sTab, sObs, sSt, sStash); else step_body<1, 2, 0, 1, 0, 0>(B, P, sTab, sObs, sSt, sStash); }
}

template <int NOBS, int POLICY> struct PolicySmem { MlpSmem<NOBS> M; };
template <int NOBS> struct PolicySmem<NOBS, LM_POLICY_GNN> { GnnSmem M; };

// Evaluation builds (lm_engine_ev.hip): template flag EV of k_rollout_ev / k_rollout_mlp_ev
#define LM_EV_DET 1      // the policy tile's mean-action epilogue (lm_rollout_set_deterministic)
#define LM_EV_REC 2      // the episode record (lm_rollout_set_episode_record)
struct RolloutEv { float* record; int cap; };
// launches the evaluation build for ev = LM_EV_DET | LM_EV_REC bits (lm_engine_ev.hip); 0, or -1 when there is no such build
extern "C" __attribute__((visibility("hidden"))) int lm_internal_launch_rollout_ev(const StepArgs* A, const RolloutDev* D, const RolloutEv* E, int ev, int policy, int nobs,
                                                                                  int nblocks, hipStream_t s);
