// lm_rollout_dev.h -- what the persistent rollout kernels share.  For all of them (k_rollout, k_rollout_mlp of lm_engine.hip and their evaluation
// and trajectory builds): the device-side argument block, the step as the stepping wavefront runs it, the policy tile's LDS.  For the evaluation
// builds (lm_engine_ev.hip) and the builds that keep a trajectory record (lm_engine_tr.hip): their argument blocks, the declarations of their
// launchers (the host side of lm_engine.hip sees them here) and their one device body, which those two units instantiate behind the template flag EV.
// The training kernels of lm_engine.hip keep a body of their own: written as EV = 0 wrappers of this one they compile differently.
#pragma once
#include "../../include/lm_policy.h"
#include "lm_policy_dev.h"
#include "lm_step.h"
#include "lm_traj_dev.h"      // LM_EV_TRAJ, RolloutTraj, traj_state_row

struct RolloutDev {
  const float* params; const float* log_std;
  float *obs, *actions, *logp, *values, *rewards; int64_t* dones;
  long long* acc_steps; int T; uint32_t noise_seed;
};

// the step of the persistent kernels: step_body is forceinline like all device code here, so the kernels' assembly holds no call (no s_swappc_b64;
// the kernels are the only functions of their units) - the step's kinds are inlined into the stepping wavefront's branch, and the stepping and
// the policy wavefronts share one register allocation, the kernel's (505 - 512 registers, VGPRs and AGPRs together)
// (last template argument 0: both passes of a sub-step read the stash, lm_dynamics.h - on registers the first pass costs these kernels, which sit at
// 512 registers, 130-190 B more scratch)
LM_DEV void step_dispatch(const StepArgs& B, const lm_params* P, float* sTab, float* sObs, float* sSt, float4* sStash) {
  if (P->variant == 0) { if (P->mode == LM_MODE_LOCO) step_body<0, 0, 0, 1, 0, 0>(B, P, sTab, sObs, sSt, sStash); else step_body<1, 0, 0, 1, 0, 0>(B, P, sTab, sObs, sSt, sStash); }
  else if (P->variant == 1) { if (P->mode == LM_MODE_LOCO) step_body<0, 1, 0, 1, 0, 0>(B, P, sTab, sObs, sSt, sStash); else step_body<1, 1, 0, 1, 0, 0>(B, P, sTab, sObs, sSt, sStash); }
  else { if (P->mode == LM_MODE_LOCO) step_body<0, 2, 0, 1, 0, 0>(B, P, sTab, sObs, sSt, sStash); else step_body<1, 2, 0, 1, 0, 0>(B, P, sTab, sObs, sSt, sStash); }
}

template <int NOBS, int POLICY> struct PolicySmem { MlpSmem<NOBS> M; };
template <int NOBS> struct PolicySmem<NOBS, LM_POLICY_GNN> { GnnSmem M; };

// ---- Evaluation and trajectory builds: template flag EV of k_rollout_ev / k_rollout_mlp_ev (lm_engine_ev.hip) and k_rollout_mlp_tr
// (lm_engine_tr.hip); the third bit, LM_EV_TRAJ, and RolloutTraj are in lm_traj_dev.h
#define LM_EV_DET 1      // the policy tile's mean-action epilogue (lm_rollout_set_deterministic)
#define LM_EV_REC 2      // the episode record (lm_rollout_set_episode_record)
struct RolloutEv { float* record; int cap; };
// launches the evaluation build for ev = LM_EV_DET | LM_EV_REC bits (lm_engine_ev.hip); 0, or -1 when there is no such build
extern "C" __attribute__((visibility("hidden"))) int lm_internal_launch_rollout_ev(const StepArgs* A, const RolloutDev* D, const RolloutEv* E, int ev, int policy, int nobs,
                                                                                  int nblocks, hipStream_t s);
// 1 when lm_engine_tr.hip has a build for these ev bits (LM_EV_TRAJ among them) / policy / observation width
extern "C" __attribute__((visibility("hidden"))) int lm_internal_rollout_tr_built(int ev, int policy, int nobs);
// launches it: 0, or -1 when there is no such build
extern "C" __attribute__((visibility("hidden"))) int lm_internal_launch_rollout_tr(const StepArgs* A, const RolloutDev* D, const RolloutEv* E, const RolloutTraj* TJ, int ev,
                                                                                  int policy, int nobs, int nblocks, hipStream_t s);

// The two records are kept by policy wavefronts, never by the stepping one.  The stepping wavefront is at its register limit (a first version
// that updated the episode record there needed 20 bytes of scratch on the 64-wide MLP build), so its loop below is that of k_rollout_mlp, and
// what a record needs of a step is read back from memory behind the block barrier that ends the step.
// Ordering, for both records.  What is read was stored by the stepping wavefront during step k; it drains its stores to the L2 (vmcnt(0)) ahead
// of the barrier that ends the step, and the loads are device-scope, so they see the L2.  The next step cannot overwrite the state rows, the
// counters or goal_reset_buf while they are being read: the stepping wavefront starts step k + 1 behind the MLP_RES_BARRIERS barriers of forward
// k + 1, and a recording wavefront enters the first of them only after every load has returned - the episode record's feed episode_update, the
// trajectory record's are the data of the row stores it has issued by then.  rewards[k] and dones[k] are never written again during the run.

// ---- the episode record: the block's 16 columns live in LDS for the rollout; lane e of the first policy wavefront owns env e's column (loaded
// on entry, stored on exit) and after a step applies episode_update (lm_policy_dev.h) to what the step stored: rewards[k], dones[k], goal_reset_buf
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

// ---- the trajectory record.  A block steps envs env0 .. env0 + 15, so at most 16 of the K tracked ids (they are distinct) are its own.  The third
// policy wavefront (P = 2: it keeps the fewest resident weights, 288 words per lane against 320 / 304) finds them once at kernel entry - a ballot
// over the id list, 64 ids at a time - and keeps per own slot the slot index, the env and the slot's four header words in LDS for the whole rollout;
// it stores the headers on exit.  After the block barrier that ends step k it walks its slots: lane = column reads the word it copies (a state row,
// rewards[k], dones[k] or a counter row) with a device-scope load and the wavefront stores the row as one contiguous 256-byte segment; lane 0 then
// moves the header in LDS (the other lanes read it again only behind the barriers of the next forward).
// sTr: int [TRAJ_BLOCK_SLOTS][TR_WORDS] = { slot, env, header words 0..3 } and the number of own slots in sTr[TR_WORDS * TRAJ_BLOCK_SLOTS]
#define TRAJ_BLOCK_SLOTS ENVS_PER_WAVE      // distinct ids: a block of 16 envs owns at most 16 slots
#define TR_WORDS 6
LM_DEV void rollout_traj_find(const RolloutTraj& TJ, int* sTr, int N, int env0, int lane) {
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
LM_DEV void rollout_traj_store(const RolloutTraj& TJ, const int* sTr, int lane) {
  if (lane < sTr[TR_WORDS * TRAJ_BLOCK_SLOTS]) {
    const size_t slot = (size_t)sTr[TR_WORDS * lane];
#pragma unroll
    for (int q = 0; q < 4; q++) TJ.header[4 * slot + q] = sTr[TR_WORDS * lane + 2 + q];
  }
}
// step k is done and its stores are in the L2 (the block barrier behind the stepping wavefront's vmcnt(0) has been passed)
LM_DEV void rollout_traj_step(const RolloutTraj& TJ, int* sTr, const float* state, const int64_t* cnt, const float* rewards_k, const int64_t* dones_k, int N, int fb, int lane) {
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

// ---- the wavefront-specialised body (k_rollout_mlp of lm_engine.hip with the flag threaded through; no diagnostic stamps: the units that
// instantiate it #undef LM_STAMPS).  The names end in _ev: lm_engine.hip includes this header and has a rollout_policy_loop of its own.
template <int NOBS, int P, int EV>
LM_DEV void rollout_policy_loop_ev(const StepArgs& A, const RolloutDev& R, const lm_params* P_, float* sObs, MlpSmem<NOBS>& M, int env0, int tp,
                                   const RolloutEv& E, float* sRec, const RolloutTraj& TJ, int* sTr) {
  // the first policy wavefront keeps the episode record, the third one the trajectory record; the mean-action epilogue is the tile's
  constexpr bool DET = (EV & LM_EV_DET) != 0, REC = (EV & LM_EV_REC) != 0 && P == 0, TRAJ = (EV & LM_EV_TRAJ) != 0 && P == 2;
  if (REC) rollout_record_load(E, sRec, A.N, env0, tp & 63);
  if (TRAJ) rollout_traj_find(TJ, sTr, A.N, env0, tp & 63);
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
    if (REC) rollout_record_step(E, sRec, R.rewards + (size_t)k * N, R.dones + (size_t)k * N, A.cnt, A.N, env0, tp & 63, P_->max_episode);
    if (TRAJ) rollout_traj_step(TJ, sTr, A.state, A.cnt, R.rewards + (size_t)k * N, R.dones + (size_t)k * N, A.N, fb, tp & 63);
  }
  if (REC) rollout_record_store(E, sRec, A.N, env0, tp & 63);
  if (TRAJ) rollout_traj_store(TJ, sTr, tp & 63);
}

template <int NOBS, int EV>
LM_DEV void rollout_mlp_block_ev(const StepArgs& A, const RolloutDev& R, const RolloutEv& E, const RolloutTraj& TJ) {
  __shared__ __attribute__((aligned(16))) float sTab[LM_ITAB_FLOATS + 2];
  __shared__ __attribute__((aligned(16))) float sObs[ENVS_PER_WAVE * LM_MAX_OBS];
  __shared__ __attribute__((aligned(16))) float sSt[ENVS_PER_WAVE * 93];
  __shared__ float4 sStash[STASH_SLOTS * 64];
  __shared__ MlpSmem<NOBS> M;
  __shared__ float sRec[(EV & LM_EV_REC) ? LM_EPISODE_ROWS * ENVS_PER_WAVE : 1];
  __shared__ int sTr[(EV & LM_EV_TRAJ) ? TR_WORDS * TRAJ_BLOCK_SLOTS + 1 : 1];
  const int t = threadIdx.x, env0 = lm_block() * ENVS_PER_WAVE;
  const lm_params* P = A.params + ((env0 >= A.split) ? 1 : 0);
  if (t < 64) {
    for (int k = 0; k <= R.T; k++) {
#pragma unroll
      for (int b = 0; b < MLP_RES_BARRIERS; b++) lds_barrier();      // the policy wavefronts' forward k: as many barriers as mlp_res_tile passes
      if (k == R.T) break;
      // (as in k_rollout: the loop body compiled like a stand-alone kernel)
      int z = 0; asm volatile("" : "+s"(z));
      StepArgs B = A; B.state = A.state + z; B.cnt = A.cnt + z; B.N = A.N + z;
      const lm_params* Pk = P + z; const size_t Nk = (size_t)B.N;
      B.actions = R.actions + (size_t)k * Nk * 12; B.goal_rand = nullptr;
      B.W.out_obs = R.obs + (size_t)(k + 1) * Nk * NOBS; B.W.out_states = nullptr; B.W.out_rew = R.rewards + (size_t)k * Nk;
      B.W.out_resets = R.dones + (size_t)k * Nk; B.W.out_extras = nullptr; B.W.acc = R.acc_steps + 16 * k;
      step_dispatch(B, Pk, sTab, sObs, sSt, sStash);
      // vmcnt(0): the step's stores are in the L2 before the barrier lets the policy wavefronts read them with device-scope loads.  Three readers
      // depend on it: the sampling of forward k + 1 (the counters key the next action noise), the episode record (rewards[k], dones[k],
      // goal_reset_buf) and the trajectory record (state rows, rewards[k], dones[k], counter rows)
      __builtin_amdgcn_s_waitcnt(0x0F70);
      lds_barrier();
    }
  } else {
    const int tp = t - 64;
    if (tp < 64) rollout_policy_loop_ev<NOBS, 0, EV>(A, R, P, sObs, M, env0, tp, E, sRec, TJ, sTr);
    else if (tp < 128) rollout_policy_loop_ev<NOBS, 1, EV>(A, R, P, sObs, M, env0, tp, E, sRec, TJ, sTr);
    else rollout_policy_loop_ev<NOBS, 2, EV>(A, R, P, sObs, M, env0, tp, E, sRec, TJ, sTr);
  }
}

// ---- the four-wavefront body (k_rollout of lm_engine.hip with the flag threaded through): every wavefront runs the policy tile, wavefront 0 the
// step.  LM_EV_DET only - the records need the specialised body above
template <int NOBS, int POLICY, int EV>
LM_DEV void rollout_block_ev(const StepArgs& A, const RolloutDev& R) {
  __shared__ __attribute__((aligned(16))) float sTab[LM_ITAB_FLOATS + 2];
  __shared__ __attribute__((aligned(16))) float sObs[ENVS_PER_WAVE * LM_MAX_OBS];
  __shared__ __attribute__((aligned(16))) float sSt[ENVS_PER_WAVE * 93];
  __shared__ float4 sStash[STASH_SLOTS * 64];
  __shared__ PolicySmem<NOBS, POLICY> PS;
  static_assert(!(EV & (LM_EV_REC | LM_EV_TRAJ)), "no recording build of the four-wavefront tile (it needs scratch memory): recording plans take the graph");
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
