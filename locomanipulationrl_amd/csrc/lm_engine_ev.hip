// Third translation unit of liblm_engine.so: the evaluation builds of the two persistent rollout kernels (k_rollout_ev, k_rollout_mlp_ev; template
// flag EV): LM_EV_DET = the policy tile's mean-action epilogue (lm_rollout_set_deterministic), LM_EV_REC = the episode record
// (lm_rollout_set_episode_record).  Kernels of their own, as the *_cf step kernels are - a plan with both switches off launches k_rollout /
// k_rollout_mlp - and a unit of their own, as k_step_w2 is: with these instantiations in lm_engine.hip the compiler laid k_rollout_mlp out differently,
// although its source had not changed.  The bodies are those of lm_engine.hip with the flag threaded through (no diagnostic stamps here).
// Instantiated: LM_EV_DET for every policy / width; LM_EV_REC only where it builds without scratch memory, the resident MLP tile on 64-wide
// observations (lm_internal_rollout_records).
// The record: the block's 16 columns live in LDS for the rollout, owned by the first 16 lanes of the first policy wavefront (lane e
// owns env e: loaded on entry, stored on exit).  The stepping wavefront is at its register limit and its code stays what it is; after its
// step - its stores drained to the L2 (vmcnt(0)) ahead of the block barrier that ends the step - the owner lane reads back what the step
// stored (rewards[t], dones[t], goal_reset_buf) with device-scope loads and applies episode_update (lm_policy_dev.h).  The next step cannot
// overwrite goal_reset_buf earlier: it starts behind the barriers of the next forward, which the owner reaches only after its loads returned.
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

LM_DEV void rollout_record_load(const RolloutEv& E, float* sRec, int N, int env0, int lane) {
  if (lane < ENVS_PER_WAVE) {
#pragma unroll
    for (int q = 0; q < LM_EPISODE_ROWS; q++) sRec[q * ENVS_PER_WAVE + lane] = (env0 + lane < N) ? E.record[(size_t)q * N + env0 + lane] : 0.f;
  }
}
LM_DEV void rollout_record_store(const RolloutEv& E, const float* sRec, int N, int env0, int lane) {
  if (lane < ENVS_PER_WAVE && env0 + lane < N) {
#pragma unroll
    for (int q = 0; q < LM_EPISODE_ROWS; q++) E.record[(size_t)q * N + env0 + lane] = sRec[q * ENVS_PER_WAVE + lane];
  }
}
// step k is done and its stores are in the L2 (the block barrier behind the stepping wavefront's vmcnt(0) has been passed)
LM_DEV void rollout_record_step(const RolloutEv& E, float* sRec, const float* rewards_k, const int64_t* dones_k, const int64_t* cnt, int N, int env0, int lane, int max_episode) {
  if (lane < ENVS_PER_WAVE && env0 + lane < N) {
    const int env = env0 + lane;
    const uint32_t rb = __hip_atomic_load(reinterpret_cast<const uint32_t*>(rewards_k) + env, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const long long d = __hip_atomic_load(reinterpret_cast<const long long*>(dones_k) + env, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const long long g = __hip_atomic_load(reinterpret_cast<const long long*>(cnt) + 2 * (size_t)N + env, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    episode_update(sRec, ENVS_PER_WAVE, lane, __builtin_bit_cast(float, rb), d != 0, g != 0, max_episode, E.cap);
  }
}

template <int NOBS, int POLICY, int EV>
LM_DEV void rollout_block(const StepArgs& A, const RolloutDev& R) {
  __shared__ __attribute__((aligned(16))) float sTab[LM_ITAB_FLOATS + 2];
  __shared__ __attribute__((aligned(16))) float sObs[ENVS_PER_WAVE * LM_MAX_OBS];
  __shared__ __attribute__((aligned(16))) float sSt[ENVS_PER_WAVE * 93];
  __shared__ float4 sStash[STASH_SLOTS * 64];
  __shared__ PolicySmem<NOBS, POLICY> PS;
  static_assert(!(EV & LM_EV_REC), "no recording build of the four-wavefront tile (it needs scratch memory): recording plans take the graph");
  constexpr bool DET = (EV & LM_EV_DET) != 0;
  const int t = threadIdx.x, env0 = lm_block() * ENVS_PER_WAVE;
  const lm_params* P = A.params + ((env0 >= A.split) ? 1 : 0);
  for (int k = 0; k <= R.T; k++) {
    // The loop body must be compiled like a stand-alone kernel: without these opaque copies the compiler hoists every loop-invariant
    // address (one 64-bit pointer per state row and per weight chunk) out of the loop and spills hundreds of registers to scratch.
    int z = 0; asm volatile("" : "+s"(z));      // an opaque zero, new in every iteration
    StepArgs B = A; B.state = A.state + z; B.cnt = A.cnt + z; B.N = A.N + z;
    const float* Wk = R.params + z; const lm_params* Pk = P + z;
    const size_t Nk = (size_t)B.N;
    SampleArgs SA{};
    if (k < R.T) { SA.log_std = R.log_std; SA.cnt = B.cnt; SA.seed = R.noise_seed; SA.actions = R.actions + (size_t)k * Nk * 12; SA.logp = R.logp + (size_t)k * Nk; }
    if (POLICY == LM_POLICY_GNN) {
      if (k == 0) gnn_block<false, DET>(R.obs, 0.f, B.N, env0, Wk, nullptr, R.values, SA, reinterpret_cast<GnnSmem&>(PS.M), t);
      else gnn_block<true, DET>(sObs, Pk->clip_obs, B.N, env0, Wk, nullptr, R.values + (size_t)k * Nk, SA, reinterpret_cast<GnnSmem&>(PS.M), t);
    } else {
      if (k == 0) mlp_block<NOBS, false, DET>(R.obs, 0.f, B.N, env0, Wk, nullptr, R.values, SA, reinterpret_cast<MlpSmem<NOBS>&>(PS.M), t);
      else mlp_block<NOBS, true, DET>(sObs, Pk->clip_obs, B.N, env0, Wk, nullptr, R.values + (size_t)k * Nk, SA, reinterpret_cast<MlpSmem<NOBS>&>(PS.M), t);
    }
    if (k == R.T) break;
    if (t < 64) {
      // (the counters and the state are written and read back by this same wavefront: program order.  The sampled actions too with the MLP;
      // the GNN tile stores them from all four wavefronts and drains those stores before its closing barrier, lm_policy_dev.h gnn_body)
      B.actions = SA.actions; B.goal_rand = nullptr;
      B.W.out_obs = R.obs + (size_t)(k + 1) * Nk * NOBS; B.W.out_states = nullptr; B.W.out_rew = R.rewards + (size_t)k * Nk;
      B.W.out_resets = R.dones + (size_t)k * Nk; B.W.out_extras = nullptr; B.W.acc = R.acc_steps + 16 * k;
      step_dispatch(B, Pk, sTab, sObs, sSt, sStash);
    }
    lds_barrier();          // the observations staged in LDS are visible to the other wavefronts; global data is private to wavefront 0
  }
}
template <int NOBS, int POLICY, int EV>
__global__ void __launch_bounds__(256) k_rollout_ev(StepArgs A, RolloutDev R, RolloutEv) { rollout_block<NOBS, POLICY, EV>(A, R); }

template <int NOBS, int P, int EV>
LM_DEV void rollout_policy_loop_ev(const StepArgs& A, const RolloutDev& R, const lm_params* P_, float* sObs, MlpSmem<NOBS>& M, int env0, int tp,
                                   const RolloutEv& E, float* sRec) {
  constexpr bool DET = (EV & LM_EV_DET) != 0, REC = (EV & LM_EV_REC) != 0 && P == 0;      // the first policy wavefront keeps the episode record
  if (REC) rollout_record_load(E, sRec, A.N, env0, tp & 63);
  MlpResRegs<NOBS, P> RG; RG.load(R.params, tp & 63, (tp & 63) >> 4);
  const size_t N = (size_t)A.N;
  const float clip_obs = P_->clip_obs;
  for (int k = 0; k <= R.T; k++) {
    SampleArgs SA{};
    if (k < R.T) { SA.log_std = R.log_std; SA.cnt = A.cnt; SA.seed = R.noise_seed; SA.actions = R.actions + (size_t)k * N * 12; SA.logp = R.logp + (size_t)k * N; }
    if (k == 0) mlp_res_tile<NOBS, P, false, DET>(R.obs, 0.f, A.N, env0, R.params, RG, R.values, SA, M, tp);
    else mlp_res_tile<NOBS, P, true, DET>(sObs, clip_obs, A.N, env0, R.params, RG, R.values + (size_t)k * N, SA, M, tp);
    if (k == R.T) break;
    lds_barrier();          // the physics step of this iteration is done: observations in LDS, counters in memory
    if (REC) rollout_record_step(E, sRec, R.rewards + (size_t)k * N, R.dones + (size_t)k * N, A.cnt, A.N, env0, tp & 63, P_->max_episode);
  }
  if (REC) rollout_record_store(E, sRec, A.N, env0, tp & 63);
}

template <int NOBS, int EV>
LM_DEV void rollout_mlp_block(const StepArgs& A, const RolloutDev& R, const RolloutEv& E) {
  __shared__ __attribute__((aligned(16))) float sTab[LM_ITAB_FLOATS + 2];
  __shared__ __attribute__((aligned(16))) float sObs[ENVS_PER_WAVE * LM_MAX_OBS];
  __shared__ __attribute__((aligned(16))) float sSt[ENVS_PER_WAVE * 93];
  __shared__ float4 sStash[STASH_SLOTS * 64];
  __shared__ MlpSmem<NOBS> M;
  __shared__ float sRec[(EV & LM_EV_REC) ? LM_EPISODE_ROWS * ENVS_PER_WAVE : 1];
  const int t = threadIdx.x, env0 = lm_block() * ENVS_PER_WAVE;
  const lm_params* P = A.params + ((env0 >= A.split) ? 1 : 0);
  if (t < 64) {
    for (int k = 0; k <= R.T; k++) {
#pragma unroll
      for (int b = 0; b < MLP_RES_BARRIERS; b++) lds_barrier();      // the policy wavefronts' forward k
      if (k == R.T) break;
      // (as in k_rollout: the loop body compiled like a stand-alone kernel)
      int z = 0; asm volatile("" : "+s"(z));
      StepArgs B = A; B.state = A.state + z; B.cnt = A.cnt + z; B.N = A.N + z;
      const lm_params* Pk = P + z; const size_t Nk = (size_t)B.N;
      B.actions = R.actions + (size_t)k * Nk * 12; B.goal_rand = nullptr;
      B.W.out_obs = R.obs + (size_t)(k + 1) * Nk * NOBS; B.W.out_states = nullptr; B.W.out_rew = R.rewards + (size_t)k * Nk;
      B.W.out_resets = R.dones + (size_t)k * Nk; B.W.out_extras = nullptr; B.W.acc = R.acc_steps + 16 * k;
      step_dispatch(B, Pk, sTab, sObs, sSt, sStash);
      __builtin_amdgcn_s_waitcnt(0x0F70);      // the counters that key the next action noise are in the L2 before the sampling wavefront reads them
      lds_barrier();
    }
  } else {
    const int tp = t - 64;
    if (tp < 64) rollout_policy_loop_ev<NOBS, 0, EV>(A, R, P, sObs, M, env0, tp, E, sRec);
    else if (tp < 128) rollout_policy_loop_ev<NOBS, 1, EV>(A, R, P, sObs, M, env0, tp, E, sRec);
    else rollout_policy_loop_ev<NOBS, 2, EV>(A, R, P, sObs, M, env0, tp, E, sRec);
  }
}
template <int NOBS, int EV>
__global__ void __launch_bounds__(256) k_rollout_mlp_ev(StepArgs A, RolloutDev R, RolloutEv E) { rollout_mlp_block<NOBS, EV>(A, R, E); }

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
