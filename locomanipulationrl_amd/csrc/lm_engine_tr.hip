// Fourth rollout translation unit of liblm_engine.so: the builds of the persistent MLP rollout kernel that keep a TRAJECTORY record
// (lm_rollout_set_trajectory_record, include/lm_policy.h): k_rollout_mlp_tr<64, EV> with LM_EV_TRAJ in EV, alone or with LM_EV_DET and / or
// LM_EV_REC of lm_engine_ev.hip.  Kernels of their own and a unit of their own, for the reason lm_engine_ev.hip is one: the persistent kernels call
// the step as a real function, and another instantiation in a unit moves the code of its neighbours.  The body is that of k_rollout_mlp_ev with
// the third flag threaded through; the stepping wavefront stays as it is.  The record's arguments travel in RolloutTraj, next to RolloutEv.
// Instantiated: the resident MLP tile on 64-wide observations only, and only the combinations that build with 0 bytes of scratch memory
// (lm_internal_rollout_tr_built; the figures are in DESIGN.md 5.3.1).  Every other plan with a trajectory record attached takes the graph.
//
// The trajectory record here.  A block steps envs env0 .. env0 + 15, so at most 16 of the K tracked ids (they are distinct) are its own.  The third
// policy wavefront (P = 2: it keeps the fewest resident weights, 288 words per lane against 320 / 304) finds them once at kernel entry - a ballot
// over the id list, 64 ids at a time - and keeps per own slot the slot index, the env and the slot's four header words in LDS for the whole rollout;
// it stores the headers on exit.  After the block barrier that ends step k it walks its slots: lane = column reads the word it copies (a state row,
// rewards[k], dones[k] or a counter row) with a device-scope load and the wavefront stores the row as one contiguous 256-byte segment; lane 0 then
// moves the header in LDS (the other lanes read it again only behind the barriers of the next forward).
// Ordering.  What is read was stored by the stepping wavefront during step k; it drains its stores to the L2 (vmcnt(0)) ahead of the barrier that
// ends the step, and the loads are device-scope, so they see the L2.  The next step cannot overwrite the state rows, the counters or goal_reset_buf
// while they are being read: the stepping wavefront starts step k + 1 behind the five barriers of forward k + 1, and the recording wavefront enters
// the first of them only after it has issued its row stores, whose data are the loaded words - every load has returned by then.  rewards[k] and
// dones[k] are never written again during the run.  The same argument carries the episode record of lm_engine_ev.hip (first policy wavefront).
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
#include "lm_traj_dev.h"

#define TRAJ_BLOCK_SLOTS ENVS_PER_WAVE      // distinct ids: a block of 16 envs owns at most 16 slots

// ---- the episode record, as in lm_engine_ev.hip (lane e of the first policy wavefront owns env e's column in LDS)
LM_DEV void tr_record_load(const RolloutEv& E, float* sRec, int N, int env0, int lane) {
  if (lane < ENVS_PER_WAVE) {
#pragma unroll
    for (int q = 0; q < LM_EPISODE_ROWS; q++) sRec[q * ENVS_PER_WAVE + lane] = (env0 + lane < N) ? E.record[(size_t)q * N + env0 + lane] : 0.f;
  }
}
LM_DEV void tr_record_store(const RolloutEv& E, const float* sRec, int N, int env0, int lane) {
  if (lane < ENVS_PER_WAVE && env0 + lane < N) {
#pragma unroll
    for (int q = 0; q < LM_EPISODE_ROWS; q++) E.record[(size_t)q * N + env0 + lane] = sRec[q * ENVS_PER_WAVE + lane];
  }
}
LM_DEV void tr_record_step(const RolloutEv& E, float* sRec, const float* rewards_k, const int64_t* dones_k, const int64_t* cnt, int N, int env0, int lane, int max_episode) {
  if (lane < ENVS_PER_WAVE && env0 + lane < N) {
    const int env = env0 + lane;
    const uint32_t rb = __hip_atomic_load(reinterpret_cast<const uint32_t*>(rewards_k) + env, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const long long d = __hip_atomic_load(reinterpret_cast<const long long*>(dones_k) + env, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const long long g = __hip_atomic_load(reinterpret_cast<const long long*>(cnt) + 2 * (size_t)N + env, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    episode_update(sRec, ENVS_PER_WAVE, lane, __builtin_bit_cast(float, rb), d != 0, g != 0, max_episode, E.cap);
  }
}

// ---- the trajectory record.  sTr: int [TRAJ_BLOCK_SLOTS][6] = { slot, env, header words 0..3 } and the number of own slots in sTr[6 * TRAJ_BLOCK_SLOTS]
#define TR_WORDS 6
LM_DEV void tr_traj_find(const RolloutTraj& TJ, int* sTr, int N, int env0, int lane) {
  int found = 0;
  for (int i0 = 0; i0 < TJ.K; i0 += 64) {
    const int i = i0 + lane;
    const int env = i < TJ.K ? TJ.ids[i] : -1;
    const bool own = env >= env0 && env < env0 + ENVS_PER_WAVE && env < N;
    const unsigned long long m = __ballot(own);
    const int pos = found + __popcll(m & ((1ull << lane) - 1ull));
    if (own && pos < TRAJ_BLOCK_SLOTS) {
      sTr[TR_WORDS * pos] = i; sTr[TR_WORDS * pos + 1] = env;
#pragma unroll
      for (int q = 0; q < 4; q++) sTr[TR_WORDS * pos + 2 + q] = TJ.header[4 * (size_t)i + q];
    }
    found += __popcll(m);
  }
  if (lane == 0) sTr[TR_WORDS * TRAJ_BLOCK_SLOTS] = found < TRAJ_BLOCK_SLOTS ? found : TRAJ_BLOCK_SLOTS;
}
LM_DEV void tr_traj_store(const RolloutTraj& TJ, const int* sTr, int lane) {
  if (lane < sTr[TR_WORDS * TRAJ_BLOCK_SLOTS]) {
    const size_t slot = (size_t)sTr[TR_WORDS * lane];
#pragma unroll
    for (int q = 0; q < 4; q++) TJ.header[4 * slot + q] = sTr[TR_WORDS * lane + 2 + q];
  }
}
// step k is done and its stores are in the L2 (the block barrier behind the stepping wavefront's vmcnt(0) has been passed)
LM_DEV void tr_traj_step(const RolloutTraj& TJ, int* sTr, const float* state, const int64_t* cnt, const float* rewards_k, const int64_t* dones_k, int N, int fb, int lane) {
  const int count = __builtin_amdgcn_readfirstlane(sTr[TR_WORDS * TRAJ_BLOCK_SLOTS]);
  const int sr = traj_state_row(lane, fb);
  for (int s = 0; s < count; s++) {
    const int slot = __builtin_amdgcn_readfirstlane(sTr[TR_WORDS * s]), env = __builtin_amdgcn_readfirstlane(sTr[TR_WORDS * s + 1]);
    const int nrows = __builtin_amdgcn_readfirstlane(sTr[TR_WORDS * s + 2]), episodes = __builtin_amdgcn_readfirstlane(sTr[TR_WORDS * s + 3]);
    if (TJ.cap > 0 && episodes >= TJ.cap) continue;
    const long long d = __hip_atomic_load(reinterpret_cast<const long long*>(dones_k) + env, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool room = nrows >= 0 && nrows < TJ.max_rows;
    if (room) {
      float v;
      if (lane < 60) {
        const uint32_t* p = lane < 59 ? reinterpret_cast<const uint32_t*>(state) + (size_t)sr * N + env : reinterpret_cast<const uint32_t*>(rewards_k) + env;
        v = __builtin_bit_cast(float, __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      } else if (lane == 60) v = d != 0 ? 1.0f : 0.0f;
      else {
        const long long w = __hip_atomic_load(reinterpret_cast<const long long*>(cnt) + (size_t)(lane == 61 ? 2 : lane == 62 ? 4 : 5) * N + env, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
        v = lane == 61 ? (w != 0 ? 1.0f : 0.0f) : (float)w;
      }
      TJ.rows[((size_t)slot * TJ.max_rows + nrows) * LM_TRAJ_COLS + lane] = v;
    }
    if (lane == 0) {
      if (room) sTr[TR_WORDS * s + 2] = nrows + 1; else sTr[TR_WORDS * s + 4] += 1;
      if (d != 0) sTr[TR_WORDS * s + 3] = episodes + 1;
    }
  }
}

template <int NOBS, int P, int EV>
LM_DEV void rollout_policy_loop_tr(const StepArgs& A, const RolloutDev& R, const lm_params* P_, float* sObs, MlpSmem<NOBS>& M, int env0, int tp,
                                   const RolloutEv& E, float* sRec, const RolloutTraj& TJ, int* sTr) {
  // the first policy wavefront keeps the episode record, the third one the trajectory record
  constexpr bool DET = (EV & LM_EV_DET) != 0, REC = (EV & LM_EV_REC) != 0 && P == 0, TRAJ = (EV & LM_EV_TRAJ) != 0 && P == 2;
  if (REC) tr_record_load(E, sRec, A.N, env0, tp & 63);
  if (TRAJ) tr_traj_find(TJ, sTr, A.N, env0, tp & 63);
  MlpResRegs<NOBS, P> RG; RG.load(R.params, tp & 63, (tp & 63) >> 4);
  const size_t N = (size_t)A.N;
  const float clip_obs = P_->clip_obs;
  const int fb = P_->mode == LM_MODE_LOCO ? R_FB0 : R_FB1;
  for (int k = 0; k <= R.T; k++) {
    SampleArgs SA{};
    if (k < R.T) { SA.log_std = R.log_std; SA.cnt = A.cnt; SA.seed = R.noise_seed; SA.actions = R.actions + (size_t)k * N * 12; SA.logp = R.logp + (size_t)k * N; }
    if (k == 0) mlp_res_tile<NOBS, P, false, DET>(R.obs, 0.f, A.N, env0, R.params, RG, R.values, SA, M, tp);
    else mlp_res_tile<NOBS, P, true, DET>(sObs, clip_obs, A.N, env0, R.params, RG, R.values + (size_t)k * N, SA, M, tp);
    if (k == R.T) break;
    lds_barrier();          // the physics step of this iteration is done: observations in LDS, counters in memory
    if (REC) tr_record_step(E, sRec, R.rewards + (size_t)k * N, R.dones + (size_t)k * N, A.cnt, A.N, env0, tp & 63, P_->max_episode);
    if (TRAJ) tr_traj_step(TJ, sTr, A.state, A.cnt, R.rewards + (size_t)k * N, R.dones + (size_t)k * N, A.N, fb, tp & 63);
  }
  if (REC) tr_record_store(E, sRec, A.N, env0, tp & 63);
  if (TRAJ) tr_traj_store(TJ, sTr, tp & 63);
}

template <int NOBS, int EV>
LM_DEV void rollout_mlp_block_tr(const StepArgs& A, const RolloutDev& R, const RolloutEv& E, const RolloutTraj& TJ) {
  __shared__ __attribute__((aligned(16))) float sTab[LM_ITAB_FLOATS + 2];
  __shared__ __attribute__((aligned(16))) float sObs[ENVS_PER_WAVE * LM_MAX_OBS];
  __shared__ __attribute__((aligned(16))) float sSt[ENVS_PER_WAVE * 93];
  __shared__ float4 sStash[STASH_SLOTS * 64];
  __shared__ MlpSmem<NOBS> M;
  __shared__ float sRec[(EV & LM_EV_REC) ? LM_EPISODE_ROWS * ENVS_PER_WAVE : 1];
  __shared__ int sTr[TR_WORDS * TRAJ_BLOCK_SLOTS + 1];
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
      __builtin_amdgcn_s_waitcnt(0x0F70);      // the step's stores - state, counters, rewards, dones - are in the L2 before the recording wavefronts read them
      lds_barrier();
    }
  } else {
    const int tp = t - 64;
    if (tp < 64) rollout_policy_loop_tr<NOBS, 0, EV>(A, R, P, sObs, M, env0, tp, E, sRec, TJ, sTr);
    else if (tp < 128) rollout_policy_loop_tr<NOBS, 1, EV>(A, R, P, sObs, M, env0, tp, E, sRec, TJ, sTr);
    else rollout_policy_loop_tr<NOBS, 2, EV>(A, R, P, sObs, M, env0, tp, E, sRec, TJ, sTr);
  }
}
template <int NOBS, int EV>
__global__ void __launch_bounds__(256) k_rollout_mlp_tr(StepArgs A, RolloutDev R, RolloutEv E, RolloutTraj TJ) { rollout_mlp_block_tr<NOBS, EV>(A, R, E, TJ); }

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
