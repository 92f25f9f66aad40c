// lm_engine.hip -- MI355X (gfx950) physics-step engine: kernels + C ABI (include/lm_engine.h); the step's device code is in lm_step.h and below.
//
// Mapping: one 64-lane wavefront = 16 environments x 4 limbs ("limb per lane").  Each lane runs the
// limb-aggregate articulated-body sweep for its overconstrained module (5 bodies, one embedded
// Bennett loop, 3 independent joints); the four lanes of an env meet at the hub through DPP
// quad-permute reductions (backward sweep: articulated inertia + bias onto the hub; forward sweep:
// hub acceleration back to the limbs).  State is SoA [row][N] in HBM, the robot table sits in LDS,
// per-task constants are read through scalar loads.  DESIGN.md sections 3-5 derive every formula.
//
// Reference rows replaced: a4-a6 (reset scatter + action scaling), a7 (PhysX world.step x
// controlFrequencyInv), a8 (state read-back), a9-a11 (obs / reward / termination), a13 (plate deltas), a14 (co-train:
// two parameter blocks in one launch); 8f-1 (PD-actuator task families = template parameter VAR of the step), 8f-3 (domain
// randomisation = template parameter DR, kernel k_step_dr); reductions over envs are fused into the step.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <math.h>
#include <new>
#include "lm_math.h"
#include "lm_rng.h"
#include "../../include/lm_engine.h"
#include "../../include/lm_policy.h"
// Diagnostic build only (-DLM_STAMPS, tools/stamp_profile.sh): the stamp buffers (LM_STAMP: lm_dynamics.h) and the per-wavefront stamps of the
// persistent rollout kernels.  No stamp exists in the product build.
#ifdef LM_STAMPS
__device__ unsigned long long lm_stamp_out[1024 * 64];
__shared__ unsigned long long lm_stamp_lds[64];      // 0..15: wavefront 0 (15 = its last stamp time); 16 (w - 1) + 16 ..: policy wavefront w of k_rollout_mlp
#define LM_PSTAMP(w, k) do { __builtin_amdgcn_sched_barrier(0); unsigned long long t_; \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); __builtin_amdgcn_sched_barrier(0); \
    if ((threadIdx.x & 63) == 0) { lm_stamp_lds[16 * (w) + (k)] += t_ - lm_stamp_lds[16 * (w) + 15]; lm_stamp_lds[16 * (w) + 15] = t_; } } while (0)
#define MLP_RES_STAMP(P, k) LM_PSTAMP((P) + 1, k)
#endif
#ifdef LM_COUNT_PASS2      // diagnostic builds only (tools/pass2_count.py): wavefront-sub-steps run / of those with a second drive pass
__device__ unsigned int lm_dbg_pass2[2];
extern "C" void lm_dbg_pass2_read(unsigned int* out, int clear) {
  hipMemcpyFromSymbol(out, HIP_SYMBOL(lm_dbg_pass2), sizeof(lm_dbg_pass2));
  if (clear) { unsigned int z[2] = {0, 0}; hipMemcpyToSymbol(HIP_SYMBOL(lm_dbg_pass2), z, sizeof(z)); }
}
#endif
#include "lm_policy_dev.h"
#include "lm_internal.h"
#include "lm_step.h"      // the device code of the step: lm_samplers.h, lm_dynamics.h, lm_task.h, lm_step.h
#include "lm_rollout_dev.h"      // RolloutDev, step_dispatch, PolicySmem; RolloutEv, RolloutTraj and the launchers of lm_engine_ev.hip / lm_engine_tr.hip

// The step kernels.  One launch per step(); a wavefront picks its specialisation (task mode x actuator family) from the kernel arguments.  The
// velocity-drive tasks (k_step: the headline) and the PD-actuator families (k_step_pd) are separate kernels, so that the register allocation
// and code layout of the one do not move when the other is edited; both blocks of a co-training engine are of one actuator family (lm_create).
__global__ void __launch_bounds__(64) LM_STEP_ATTR k_step(StepArgs A) {                 // velocity-drive tasks (kinds 0, 1)
  LM_STEP_SMEM(64)
  LM_STEP_PROLOGUE
  if (kind == 0) step_body<0, 0, 0>(A, P, sTab, sObs, sSt, sStash); else step_body<1, 0, 0>(A, P, sTab, sObs, sSt, sStash);
  LM_STEP_EPILOGUE
}

__global__ void __launch_bounds__(64) k_step_pd(StepArgs A) {              // PD-actuator families (kinds 2 ... 5)
  LM_STEP_SMEM(LM_MAX_OBS)
  LM_STEP_PROLOGUE
  if (kind == 2) step_body<0, 1, 0>(A, P, sTab, sObs, sSt, sStash); else if (kind == 3) step_body<1, 1, 0>(A, P, sTab, sObs, sSt, sStash);
  else if (kind == 4) step_body<0, 2, 0>(A, P, sTab, sObs, sSt, sStash); else step_body<1, 2, 0>(A, P, sTab, sObs, sSt, sStash);
  LM_STEP_EPILOGUE
}

// the same steps with domain randomisation (separate kernels so that the un-randomised ones above are untouched)
__global__ void __launch_bounds__(64) k_step_dr(StepArgs A) {
  LM_STEP_SMEM(64)
  if (kind == 0) step_body<0, 0, 1>(A, P, sTab, sObs, sSt, sStash); else step_body<1, 0, 1>(A, P, sTab, sObs, sSt, sStash);
}

__global__ void __launch_bounds__(64) k_step_dr_pd(StepArgs A) {
  LM_STEP_SMEM(LM_MAX_OBS)
  if (kind == 2) step_body<0, 1, 1>(A, P, sTab, sObs, sSt, sStash); else if (kind == 3) step_body<1, 1, 1>(A, P, sTab, sObs, sSt, sStash);
  else if (kind == 4) step_body<0, 2, 1>(A, P, sTab, sObs, sSt, sStash); else step_body<1, 2, 1>(A, P, sTab, sObs, sSt, sStash);
}

// the same four kernels with contact-force reporting (lm_enable_contact_forces): kernels of their own, so that an engine that
// did not opt in runs the code above unchanged.  The randomised pair too: a wave-uniform switch inside k_step_dr / k_step_dr_pd would keep the
// four accumulators and the saved impulses allocated in kernels that already fill their 256 VGPRs and spill scalar registers, whether reporting is on or not
// (new kernels: 4 more AGPRs each; the switch would cost the kernels without reporting those too)
__global__ void __launch_bounds__(64) k_step_cf(StepArgs A) {
  LM_STEP_SMEM(64)
  if (kind == 0) step_body<0, 0, 0, 0, 1>(A, P, sTab, sObs, sSt, sStash); else step_body<1, 0, 0, 0, 1>(A, P, sTab, sObs, sSt, sStash);
}

__global__ void __launch_bounds__(64) k_step_pd_cf(StepArgs A) {
  LM_STEP_SMEM(LM_MAX_OBS)
  if (kind == 2) step_body<0, 1, 0, 0, 1>(A, P, sTab, sObs, sSt, sStash); else if (kind == 3) step_body<1, 1, 0, 0, 1>(A, P, sTab, sObs, sSt, sStash);
  else if (kind == 4) step_body<0, 2, 0, 0, 1>(A, P, sTab, sObs, sSt, sStash); else step_body<1, 2, 0, 0, 1>(A, P, sTab, sObs, sSt, sStash);
}

__global__ void __launch_bounds__(64) k_step_dr_cf(StepArgs A) {
  LM_STEP_SMEM(64)
  if (kind == 0) step_body<0, 0, 1, 0, 1>(A, P, sTab, sObs, sSt, sStash); else step_body<1, 0, 1, 0, 1>(A, P, sTab, sObs, sSt, sStash);
}

__global__ void __launch_bounds__(64) k_step_dr_pd_cf(StepArgs A) {
  LM_STEP_SMEM(LM_MAX_OBS)
  if (kind == 2) step_body<0, 1, 1, 0, 1>(A, P, sTab, sObs, sSt, sStash); else if (kind == 3) step_body<1, 1, 1, 0, 1>(A, P, sTab, sObs, sSt, sStash);
  else if (kind == 4) step_body<0, 2, 1, 0, 1>(A, P, sTab, sObs, sSt, sStash); else step_body<1, 2, 1, 0, 1>(A, P, sTab, sObs, sSt, sStash);
}

// ---- persistent rollout: T x (policy forward -> action sampling -> physics step) + the bootstrap forward without leaving
// the kernel.  A block owns its 16 envs for the whole rollout: wavefront 0 runs the step exactly as k_step does (same step_body), the
// observations it stages in LDS feed the next forward directly, and all four wavefronts run the policy tile (MLP or GNN, lm_policy_dev.h).  Blocks
// never wait for each other, so a step costs a block its own time rather than the slowest block's, and no launch boundary is paid.
// The per-step reductions go to per-step accumulators (blocks drift apart); k_rollout_finalize publishes the extras afterwards, in
// step order, with the same arithmetic as the last-arriver path of write_outputs.
template <int NOBS, int POLICY>
__global__ void __launch_bounds__(256) k_rollout(StepArgs A, RolloutDev R) {
  __shared__ __attribute__((aligned(16))) float sTab[LM_ITAB_FLOATS + 2];
  __shared__ __attribute__((aligned(16))) float sObs[ENVS_PER_WAVE * LM_MAX_OBS];
  __shared__ __attribute__((aligned(16))) float sSt[ENVS_PER_WAVE * 93];
  __shared__ float4 sStash[STASH_SLOTS * 64];
  __shared__ PolicySmem<NOBS, POLICY> PS;
  const int t = threadIdx.x, env0 = lm_block() * ENVS_PER_WAVE;
  const lm_params* P = A.params + ((env0 >= A.split) ? 1 : 0);
#ifdef LM_STAMPS
  if (threadIdx.x < 64) lm_stamp_lds[threadIdx.x] = 0;
  __builtin_amdgcn_s_waitcnt(0xc07f); __builtin_amdgcn_s_barrier();
  { unsigned long long t0_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0_) :: "memory"); if ((threadIdx.x & 63) == 0) lm_stamp_lds[16 * (threadIdx.x >> 6) + 15] = t0_; }
  __syncthreads();
#endif
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
      if (k == 0) gnn_block<false>(R.obs, 0.f, B.N, env0, Wk, nullptr, R.values, SA, reinterpret_cast<GnnSmem&>(PS.M), t);
      else gnn_block<true>(sObs, Pk->clip_obs, B.N, env0, Wk, nullptr, R.values + (size_t)k * Nk, SA, reinterpret_cast<GnnSmem&>(PS.M), t);
    } else {
      if (k == 0) mlp_block<NOBS, false>(R.obs, 0.f, B.N, env0, Wk, nullptr, R.values, SA, reinterpret_cast<MlpSmem<NOBS>&>(PS.M), t);
      else mlp_block<NOBS, true>(sObs, Pk->clip_obs, B.N, env0, Wk, nullptr, R.values + (size_t)k * Nk, SA, reinterpret_cast<MlpSmem<NOBS>&>(PS.M), t);
    }
    if (t < 64) LM_STAMP(13);      // diagnostic build: the policy tile as wavefront 0 sees it
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
    if (t < 64) LM_STAMP(14);
  }
#ifdef LM_STAMPS
  __syncthreads();
  if (threadIdx.x < 64 && blockIdx.x < 1024) lm_stamp_out[blockIdx.x * 64 + threadIdx.x] = lm_stamp_lds[threadIdx.x];
#endif
}

// ---- persistent rollout with the MLP policy: wavefront-specialised.  Wavefront 0 steps the physics; wavefronts 1..3 hold the policy's weights
// in registers for the whole rollout and run the forward + sampling between two physics steps (lm_policy_dev.h mlp_res_tile).  The two roles
// are separate loops (separate live ranges: the 300 weight registers of a policy wavefront never meet the physics' 440) that meet at block
// barriers: MLP_RES_BARRIERS inside a forward, one after the physics step (observations staged in LDS).
template <int NOBS, int P>
LM_DEV void rollout_policy_loop(const StepArgs& A, const RolloutDev& R, const lm_params* P_, float* sObs, MlpSmem<NOBS>& M, int env0, int tp) {
  MlpResRegs<NOBS, P> RG; RG.load(R.params, tp & 63, (tp & 63) >> 4);
  const size_t N = (size_t)A.N;
  const float clip_obs = P_->clip_obs;
  for (int k = 0; k <= R.T; k++) {
    SampleArgs SA{};
    if (k < R.T) { SA.log_std = R.log_std; SA.cnt = A.cnt; SA.seed = R.noise_seed; SA.actions = R.actions + (size_t)k * N * 12; SA.logp = R.logp + (size_t)k * N; }
    if (k == 0) mlp_res_tile<NOBS, P, false>(R.obs, 0.f, A.N, env0, R.params, RG, R.values, SA, M, tp);
    else mlp_res_tile<NOBS, P, true>(sObs, clip_obs, A.N, env0, R.params, RG, R.values + (size_t)k * N, SA, M, tp);
    if (k == R.T) break;
    lds_barrier();          // the physics step of this iteration is done: observations in LDS, counters in memory
  }
}

template <int NOBS>
__global__ void __launch_bounds__(256) k_rollout_mlp(StepArgs A, RolloutDev R) {
  __shared__ __attribute__((aligned(16))) float sTab[LM_ITAB_FLOATS + 2];
  __shared__ __attribute__((aligned(16))) float sObs[ENVS_PER_WAVE * LM_MAX_OBS];
  __shared__ __attribute__((aligned(16))) float sSt[ENVS_PER_WAVE * 93];
  __shared__ float4 sStash[STASH_SLOTS * 64];
  __shared__ MlpSmem<NOBS> M;
  const int t = threadIdx.x, env0 = lm_block() * ENVS_PER_WAVE;
  const lm_params* P = A.params + ((env0 >= A.split) ? 1 : 0);
#ifdef LM_STAMPS
  if (threadIdx.x < 64) lm_stamp_lds[threadIdx.x] = 0;
  __builtin_amdgcn_s_waitcnt(0xc07f); __builtin_amdgcn_s_barrier();
  { unsigned long long t0_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0_) :: "memory"); if ((threadIdx.x & 63) == 0) lm_stamp_lds[16 * (threadIdx.x >> 6) + 15] = t0_; }
  __syncthreads();
#endif
  if (t < 64) {
    for (int k = 0; k <= R.T; k++) {
#pragma unroll
      for (int b = 0; b < MLP_RES_BARRIERS; b++) lds_barrier();      // the policy wavefronts' forward k
      LM_STAMP(13);
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
      LM_STAMP(14);
    }
  } else {
    const int tp = t - 64;
    if (tp < 64) rollout_policy_loop<NOBS, 0>(A, R, P, sObs, M, env0, tp);
    else if (tp < 128) rollout_policy_loop<NOBS, 1>(A, R, P, sObs, M, env0, tp);
    else rollout_policy_loop<NOBS, 2>(A, R, P, sObs, M, env0, tp);
  }
#ifdef LM_STAMPS
  __syncthreads();
  if (threadIdx.x < 64 && blockIdx.x < 1024) lm_stamp_out[blockIdx.x * 64 + threadIdx.x] = lm_stamp_lds[threadIdx.x];
#endif
}

// extras and success windows of the T steps of a persistent rollout, in step order: the accumulator rows are fetched (and cleared) 64 steps
// at a time, the window counters live in registers across the steps; same arithmetic as publish_extra
__global__ void __launch_bounds__(64) k_rollout_finalize(const lm_params* params, OutPtrs W, int N, long long* acc_steps, float* extras, int T) {
  __shared__ long long sAcc[64 * 16];
  __shared__ int sCnt[64 * 4];          // per step: goal resets, resets (all envs), goal resets, resets (first task)
  const int lane = threadIdx.x;
  int64_t* ns_g = reinterpret_cast<int64_t*>(W.stats); float* rate_g = reinterpret_cast<float*>(W.stats + 48);
  int64_t ns[6]; float rate[3];
#pragma unroll
  for (int i = 0; i < 6; i++) ns[i] = ns_g[i];
#pragma unroll
  for (int i = 0; i < 3; i++) rate[i] = rate_g[i];
  const int64_t max_cnt = (int64_t)params->max_reset_counts;
  for (int k0 = 0; k0 < T; k0 += 64) {
    const int nk = min(64, T - k0);
    {
      // all 16 loads of a lane in flight at once (they bypass the L2: issued one by one, each was a full round trip), then the clears
      long long v[16];
#pragma unroll
      for (int j = 0; j < 16; j++) { const int i = lane + 64 * j; v[j] = (i < nk * 16) ? __hip_atomic_load(acc_steps + 16 * (size_t)k0 + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0LL; }
#pragma unroll
      for (int j = 0; j < 16; j++) { const int i = lane + 64 * j; if (i < nk * 16) { sAcc[i] = v[j]; __hip_atomic_store(acc_steps + 16 * (size_t)k0 + i, 0LL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); } }
    }
    __builtin_amdgcn_s_waitcnt(0xc07f); __builtin_amdgcn_wave_barrier();
    // the means of a step do not depend on the other steps: one lane per step (same arithmetic as publish_extra)
    if (lane < nk) {
      const bool last = (k0 + lane == T - 1);
      float* ex = extras ? extras + (size_t)(k0 + lane) * LM_NUM_EXTRAS : nullptr;
#pragma unroll
      for (int j = 0; j < 14; j++) {
        const float sum = (float)((double)sAcc[16 * lane + j] * (1.0 / (double)ACC_SCALE));
        if (j < 7) { const float m = sum / (float)N; if (last) W.extras[j] = m; if (ex) ex[j] = m; }
        else if (j >= 9 && j < 12) { const float m = sum / (float)N; if (last) W.extras[j + 1] = m; if (ex) ex[j + 1] = m; }
        else sCnt[4 * lane + (j == 7 ? 0 : j == 8 ? 1 : j == 12 ? 2 : 3)] = (int)(sum + 0.5f);
      }
    }
    __builtin_amdgcn_s_waitcnt(0xc07f); __builtin_amdgcn_wave_barrier();
    // the success-rate windows are a recurrence over the steps: one lane walks them in order
    if (lane == 0) {
      for (int k = 0; k < nk; k++) {
        const bool last = (k0 + k == T - 1);
        float* ex = extras ? extras + (size_t)(k0 + k) * LM_NUM_EXTRAS : nullptr;
        const int64_t gs = sCnt[4 * k], rs = sCnt[4 * k + 1], gl = sCnt[4 * k + 2], rl = sCnt[4 * k + 3];
        success_window(ns + 0, rate + 0, gs, rs, max_cnt);
        success_window(ns + 2, rate + 1, gl, rl, max_cnt);
        success_window(ns + 4, rate + 2, gs - gl, rs - rl, max_cnt);
#pragma unroll
        for (int c = 0; c < 3; c++) { if (last) W.extras[7 + c] = rate[c]; if (ex) ex[7 + c] = rate[c]; }
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 6; i++) ns_g[i] = ns[i];
#pragma unroll
    for (int i = 0; i < 3; i++) rate_g[i] = rate[i];
  }
}

__global__ void __launch_bounds__(64) k_reset_all(int64_t* cnt, int N) {
  int i = blockIdx.x * 64 + threadIdx.x;
  if (i < N) cnt[3 * (size_t)N + i] = 1;
}

// ---- test / tooling kernels ---------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_apply_resets(StepArgs A) {
  const int lane = threadIdx.x, limb = lane & 3, envl = lane >> 2;
  const int envr = lm_block() * ENVS_PER_WAVE + envl, N = A.N; if (envr >= N) return; const int env = envr;
  const lm_params* P = A.params + ((lm_block() * ENVS_PER_WAVE >= A.split) ? 1 : 0);
  const int jj[3] = {limb, 4 + 2 * limb, 5 + 2 * limb};
  float* st = A.state; int64_t* cnt = A.cnt;
  if (cnt[3 * (size_t)N + env] == 0) return;
  int episode = (int)cnt[5 * (size_t)N + env];
  float u3[3];
  if (A.goal_rand) { u3[0] = A.goal_rand[(size_t)env * 3]; u3[1] = A.goal_rand[(size_t)env * 3 + 1]; u3[2] = A.goal_rand[(size_t)env * 3 + 2]; }
  else hash_uniform3(A.seed, (uint32_t)env, (uint32_t)episode, u3);
  Q4 g = quat_from_euler(P->goal_lo[0] + (P->goal_hi[0] - P->goal_lo[0]) * u3[0], P->goal_lo[1] + (P->goal_hi[1] - P->goal_lo[1]) * u3[1],
                         P->goal_lo[2] + (P->goal_hi[2] - P->goal_lo[2]) * u3[2]);
  for (int a = 0; a < 3; a++) {
    st[(size_t)(R_Q + jj[a]) * N + env] = P->init_q[jj[a]]; st[(size_t)(R_QD + jj[a]) * N + env] = 0.f;
    st[(size_t)(R_LACT + jj[a]) * N + env] = 0.f; st[(size_t)(R_LQD + jj[a]) * N + env] = 0.f;
    st[(size_t)(R_LTIP + 3 * limb + a) * N + env] = P->default_tip[3 * limb + a];
    st[(size_t)(R_SE + jj[a]) * N + env] = P->init_se[jj[a]]; st[(size_t)(R_LTGT + jj[a]) * N + env] = P->init_q[jj[a]];
  }
  __builtin_amdgcn_wave_barrier();
  if (limb == 0) {
    for (int k = 0; k < 3; k++) {
      st[(size_t)(R_FB0 + k) * N + env] = P->init_base_pos[k]; st[(size_t)(R_FB0 + 7 + k) * N + env] = 0.f; st[(size_t)(R_FB0 + 10 + k) * N + env] = 0.f;
      st[(size_t)(R_FB1 + k) * N + env] = P->init_plate_pos[k]; st[(size_t)(R_FB1 + 7 + k) * N + env] = 0.f; st[(size_t)(R_FB1 + 10 + k) * N + env] = 0.f;
    }
    for (int k = 0; k < 4; k++) { st[(size_t)(R_FB0 + 3 + k) * N + env] = P->init_base_quat[k]; st[(size_t)(R_FB1 + 3 + k) * N + env] = P->init_plate_quat[k]; }
    st[(size_t)(R_GOAL + 0) * N + env] = g.w; st[(size_t)(R_GOAL + 1) * N + env] = g.x; st[(size_t)(R_GOAL + 2) * N + env] = g.y; st[(size_t)(R_GOAL + 3) * N + env] = g.z;
    const bool fixedb = (P->mode == LM_MODE_MANI);
    Q4 qb; qb.w = fixedb ? 1.f : P->init_base_quat[0]; qb.x = fixedb ? 0.f : -P->init_base_quat[1]; qb.y = fixedb ? 0.f : -P->init_base_quat[2]; qb.z = fixedb ? 0.f : -P->init_base_quat[3];
    Q4 d4 = qmul(qb, qconj(g));
    st[(size_t)R_LRD * N + env] = 2.0f * asinf(fminf(sqrtf(d4.x * d4.x + d4.y * d4.y + d4.z * d4.z), 1.0f));
  }
}
__global__ void __launch_bounds__(64) k_apply_resets_cnt(int64_t* cnt, int N) {
  int i = blockIdx.x * 64 + threadIdx.x; if (i >= N) return;
  if (cnt[3 * (size_t)N + i] != 0) { cnt[0 * (size_t)N + i] = 0; cnt[1 * (size_t)N + i] = 0; cnt[2 * (size_t)N + i] = 0; cnt[3 * (size_t)N + i] = 0; cnt[4 * (size_t)N + i] = 0; cnt[5 * (size_t)N + i] += 1; }
}

// quat_to_mat with the contraction written out the way the compiler contracts it at step_body's world -> body conversion (the w products and
// the first square of each diagonal sum are the plain multiplies).  In load_phys it contracts y z -+ w x the other way round, which moves the body twist by an ulp: enough to make the
// contact record of lm_substeps differ from lm_step's in the last bits.  k_substeps_cf loads through this one (XR = 1)
LM_DEV M3 quat_to_mat_step(float w, float x, float y, float z) {
  const float wx = w * x, wy = w * y, wz = w * z;
  M3 R;
  R.c0 = v3(fmaf(-2.f, fmaf(z, z, y * y), 1.f), 2.f * fmaf(x, y, wz), 2.f * fmaf(x, z, -wy));
  R.c1 = v3(2.f * fmaf(x, y, -wz), fmaf(-2.f, fmaf(z, z, x * x), 1.f), 2.f * fmaf(y, z, wx));
  R.c2 = v3(2.f * fmaf(x, z, wy), 2.f * fmaf(y, z, -wx), fmaf(-2.f, fmaf(y, y, x * x), 1.f));
  return R;
}
template <int MODE, int XR = 0>
LM_DEV void load_phys(const float* st, int N, int env, int limb, FreeBody& F, float q[3], float qd[3]) {
  const int fb = (MODE == 0) ? R_FB0 : R_FB1; const int jj[3] = {limb, 4 + 2 * limb, 5 + 2 * limb};
  F.p = v3(st[(size_t)(fb + 0) * N + env], st[(size_t)(fb + 1) * N + env], st[(size_t)(fb + 2) * N + env]);
  F.q.w = st[(size_t)(fb + 3) * N + env]; F.q.x = st[(size_t)(fb + 4) * N + env]; F.q.y = st[(size_t)(fb + 5) * N + env]; F.q.z = st[(size_t)(fb + 6) * N + env];
  V3 lin = v3(st[(size_t)(fb + 7) * N + env], st[(size_t)(fb + 8) * N + env], st[(size_t)(fb + 9) * N + env]);
  V3 ang = v3(st[(size_t)(fb + 10) * N + env], st[(size_t)(fb + 11) * N + env], st[(size_t)(fb + 12) * N + env]);
  M3 R = XR ? quat_to_mat_step(F.q.w, F.q.x, F.q.y, F.q.z) : quat_to_mat(F.q.w, F.q.x, F.q.y, F.q.z); F.u = sv(mulT(R, ang), mulT(R, lin));
  for (int a = 0; a < 3; a++) { q[a] = st[(size_t)(R_Q + jj[a]) * N + env]; qd[a] = st[(size_t)(R_QD + jj[a]) * N + env]; }
}
template <int MODE>
LM_DEV void store_phys(float* st, int N, int env, int limb, const FreeBody& F, const float q[3], const float qd[3]) {
  const int fb = (MODE == 0) ? R_FB0 : R_FB1; const int jj[3] = {limb, 4 + 2 * limb, 5 + 2 * limb};
  for (int a = 0; a < 3; a++) { st[(size_t)(R_Q + jj[a]) * N + env] = q[a]; st[(size_t)(R_QD + jj[a]) * N + env] = qd[a]; }
  if (limb == 0) {
    M3 R = quat_to_mat(F.q.w, F.q.x, F.q.y, F.q.z); V3 lin = mul(R, F.u.v), ang = mul(R, F.u.w);
    st[(size_t)(fb + 0) * N + env] = F.p.x; st[(size_t)(fb + 1) * N + env] = F.p.y; st[(size_t)(fb + 2) * N + env] = F.p.z;
    st[(size_t)(fb + 3) * N + env] = F.q.w; st[(size_t)(fb + 4) * N + env] = F.q.x; st[(size_t)(fb + 5) * N + env] = F.q.y; st[(size_t)(fb + 6) * N + env] = F.q.z;
    st[(size_t)(fb + 7) * N + env] = lin.x; st[(size_t)(fb + 8) * N + env] = lin.y; st[(size_t)(fb + 9) * N + env] = lin.z;
    st[(size_t)(fb + 10) * N + env] = ang.x; st[(size_t)(fb + 11) * N + env] = ang.y; st[(size_t)(fb + 12) * N + env] = ang.z;
  }
}

template <int MODE, int VAR, int CF = 0>
LM_DEV void substeps_body(const StepArgs& A, const lm_params* P, const float* sTab, const float* targets, int n, float4* sStash) {
  const int lane = threadIdx.x, limb = lane & 3, envl = lane >> 2;
  Stash St; St.base = sStash; St.lane = lane;
  const int envr = lm_block() * ENVS_PER_WAVE + envl, N = A.N; const bool active = envr < N; const int env = active ? envr : N - 1;
  const float* tl = sTab + HUB_FLOATS + limb * LIMB_STRIDE; const int jj[3] = {limb, 4 + 2 * limb, 5 + 2 * limb};
  FreeBody F; float q[3], qd[3], tgt[3];
  load_phys<MODE, CF>(A.state, N, env, limb, F, q, qd);
  for (int a = 0; a < 3; a++) tgt[a] = targets[(size_t)env * 12 + jj[a]];
  M3 Rfix = quat_to_mat(P->fixed_base_quat[0], P->fixed_base_quat[1], P->fixed_base_quat[2], P->fixed_base_quat[3]);
  V3 pfix = v3(P->fixed_base_pos[0], P->fixed_base_pos[1], P->fixed_base_pos[2]);
  float tau_acc[3] = {0.f, 0.f, 0.f};
  DrPhys X; float cf[4] = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < n; s++) substep<MODE, VAR, 0, CF>(P, sTab, tl, limb, St, F, Rfix, pfix, q, qd, tgt, tau_acc, X, cf);
  if (active) store_phys<MODE>(A.state, N, env, limb, F, q, qd);
  if (CF) store_contact(A.contact, N, env, limb, active, cf, n, P->dt);
}
__global__ void __launch_bounds__(64) k_substeps(StepArgs A, const float* targets, int n) {
  __shared__ __attribute__((aligned(16))) float sTab[LM_ITAB_FLOATS + 2];
  __shared__ float4 sStash[STASH_SLOTS * 64];
  load_table(A.table, sTab, threadIdx.x);
  const lm_params* P = A.params + ((lm_block() * ENVS_PER_WAVE >= A.split) ? 1 : 0);
  if (P->variant == 0) { if (P->mode == LM_MODE_LOCO) substeps_body<0, 0>(A, P, sTab, targets, n, sStash); else substeps_body<1, 0>(A, P, sTab, targets, n, sStash); }
  else { if (P->mode == LM_MODE_LOCO) substeps_body<0, 1>(A, P, sTab, targets, n, sStash); else substeps_body<1, 1>(A, P, sTab, targets, n, sStash); }
}

__global__ void __launch_bounds__(64) k_substeps_cf(StepArgs A, const float* targets, int n) {      // k_substeps with contact-force reporting
  __shared__ __attribute__((aligned(16))) float sTab[LM_ITAB_FLOATS + 2];
  __shared__ float4 sStash[STASH_SLOTS * 64];
  load_table(A.table, sTab, threadIdx.x);
  const lm_params* P = A.params + ((lm_block() * ENVS_PER_WAVE >= A.split) ? 1 : 0);
  if (P->variant == 0) { if (P->mode == LM_MODE_LOCO) substeps_body<0, 0, 1>(A, P, sTab, targets, n, sStash); else substeps_body<1, 0, 1>(A, P, sTab, targets, n, sStash); }
  else { if (P->mode == LM_MODE_LOCO) substeps_body<0, 1, 1>(A, P, sTab, targets, n, sStash); else substeps_body<1, 1, 1>(A, P, sTab, targets, n, sStash); }
}

__global__ void __launch_bounds__(64) k_fk(StepArgs A, float* tips, float* knees) {
  __shared__ __attribute__((aligned(16))) float sTab[LM_ITAB_FLOATS + 2];
  load_table(A.table, sTab, threadIdx.x);
  const lm_params* P = A.params + ((lm_block() * ENVS_PER_WAVE >= A.split) ? 1 : 0);
  const int lane = threadIdx.x, limb = lane & 3, envl = lane >> 2;
  const int env = lm_block() * ENVS_PER_WAVE + envl, N = A.N; if (env >= N) return;
  const float* tl = sTab + HUB_FLOATS + limb * LIMB_STRIDE;
  FreeBody F; float q[3], qd[3];
  M3 Rb; V3 pb;
  if (P->mode == LM_MODE_LOCO) { load_phys<0>(A.state, N, env, limb, F, q, qd); Rb = quat_to_mat(F.q.w, F.q.x, F.q.y, F.q.z); pb = F.p; }
  else { load_phys<1>(A.state, N, env, limb, F, q, qd); Rb = quat_to_mat(P->fixed_base_quat[0], P->fixed_base_quat[1], P->fixed_base_quat[2], P->fixed_base_quat[3]);
         pb = v3(P->fixed_base_pos[0], P->fixed_base_pos[1], P->fixed_base_pos[2]); }
  LimbKin K; float z3[3] = {0, 0, 0}; limb_kinematics(tl, q, z3, K);
  V3 xh, k2h, k3h; limb_points(tl, K, xh, k2h, k3h);
  V3 x = pb + mul(Rb, xh);
  V3 k2 = pb + mul(Rb, k2h), k3 = pb + mul(Rb, k3h);
  float* t = tips + ((size_t)env * 4 + limb) * 3; t[0] = x.x; t[1] = x.y; t[2] = x.z;
  float* kk = knees + ((size_t)env * 8 + 2 * limb) * 3; kk[0] = k2.x; kk[1] = k2.y; kk[2] = k2.z; kk[3] = k3.x; kk[4] = k3.y; kk[5] = k3.z;
}

// dense M (18x18) and h (18) of the loco system from the limb-aggregate terms (bring-up / parity tests)
__global__ void __launch_bounds__(64) k_debug_dyn(StepArgs A, float* Mout, float* hout) {
  __shared__ __attribute__((aligned(16))) float sTab[LM_ITAB_FLOATS + 2];
  load_table(A.table, sTab, threadIdx.x);
  const lm_params* P = A.params;
  const int lane = threadIdx.x, limb = lane & 3, envl = lane >> 2;
  const int envr = lm_block() * ENVS_PER_WAVE + envl, N = A.N; const bool active = envr < N; const int env = active ? envr : N - 1;
  const float* tl = sTab + HUB_FLOATS + limb * LIMB_STRIDE; const int jj[3] = {limb, 4 + 2 * limb, 5 + 2 * limb};
  FreeBody F; float q[3], qd[3];
  load_phys<0>(A.state, N, env, limb, F, q, qd);
  M3 Rb = quat_to_mat(F.q.w, F.q.x, F.q.y, F.q.z);
  SV avp0 = sv(v3(0, 0, 0), P->gravity * row2(Rb));
  LimbKin K; limb_kinematics(tl, q, qd, K);
  LimbDyn D; limb_dynamics(tl, K, qd, F.u, avp0, D);
  float Ac[6][6]; si_to_66(D.Isc, Ac);
  SI I0 = hub_inertia(sTab); float A0[6][6]; si_to_66(I0, A0);
  SV b = quad_sum(D.fcs) + I0 * avp0 + fcross(F.u, I0 * F.u);
  float* M = Mout + (size_t)env * 324; float* h = hout + (size_t)env * 18;
  float bb[6]; sv_to_arr(b, bb);
  for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) { float v = quad_sum(Ac[i][j]) + A0[i][j]; if (active && limb == 0) M[i * 18 + j] = v; }
  if (active) {
    if (limb == 0) for (int i = 0; i < 6; i++) h[i] = bb[i];
    float f[3][6]; sv_to_arr(D.Fq0, f[0]); sv_to_arr(D.Fq1, f[1]); sv_to_arr(D.Fq2, f[2]);
    const int hi[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
    for (int a = 0; a < 3; a++) {
      for (int i = 0; i < 6; i++) { M[i * 18 + 6 + jj[a]] = f[a][i]; M[(6 + jj[a]) * 18 + i] = f[a][i]; }
      for (int c = 0; c < 3; c++) M[(6 + jj[a]) * 18 + 6 + jj[c]] = D.H[hi[a][c]];
      h[6 + jj[a]] = D.hq[a];
    }
  }
}

template <int MODE>
LM_DEV void task_only_body(const StepArgs& A, const lm_params* P, const float* rb_all, float* sObs, float* sSt) {
  const int lane = threadIdx.x, limb = lane & 3, envl = lane >> 2;
  const int env0 = lm_block() * ENVS_PER_WAVE, envr = env0 + envl, N = A.N; const bool active = envr < N; const int env = active ? envr : N - 1;
  const int jj[3] = {limb, 4 + 2 * limb, 5 + 2 * limb};
  float* st = A.state; int64_t* cnt = A.cnt;
  const float* rb = rb_all + (size_t)env * 99;
  TaskIn I; TaskState S; TaskOut O;
  for (int a = 0; a < 3; a++) { I.q[a] = rb[jj[a]]; I.qd[a] = rb[12 + jj[a]]; I.acc[a] = rb[24 + jj[a]];
    I.act[a] = clampf(A.actions[(size_t)env * 12 + jj[a]], P->clip_actions); S.lact[a] = st[(size_t)(R_LACT + jj[a]) * N + env];
    I.torque[a] = rb[87 + jj[a]]; S.ltgt[a] = st[(size_t)(R_LTGT + jj[a]) * N + env]; }
  {
    // custom-controller tasks: integrate the swing / extension targets like pre_physics_step (:255-276)
    float se[3];
    for (int a = 0; a < 3; a++) { se[a] = st[(size_t)(R_SE + jj[a]) * N + env];
      if (P->variant >= 1) { se[a] = fminf(fmaxf(se[a] + I.act[a] * P->act_scale_se, P->se_lo[jj[a]]), P->se_hi[jj[a]]); if (active) st[(size_t)(R_SE + jj[a]) * N + env] = se[a]; } }
    I.tgtq[0] = se[0]; I.tgtq[1] = se[1] + 0.5f * se[2]; I.tgtq[2] = se[1] - 0.5f * se[2];
    S.lrd = st[(size_t)R_LRD * N + env];
  }
  I.fp = v3(rb[36], rb[37], rb[38]); I.fq.w = rb[39]; I.fq.x = rb[40]; I.fq.y = rb[41]; I.fq.z = rb[42];
  I.lin = v3(rb[43], rb[44], rb[45]); I.ang = v3(rb[46], rb[47], rb[48]);
  I.tipw = v3(rb[49 + 3 * limb], rb[50 + 3 * limb], rb[51 + 3 * limb]);
  I.knee2 = v3(rb[61 + 6 * limb], rb[62 + 6 * limb], rb[63 + 6 * limb]); I.knee3 = v3(rb[64 + 6 * limb], rb[65 + 6 * limb], rb[66 + 6 * limb]);
  S.ltip = v3(st[(size_t)(R_LTIP + 3 * limb) * N + env], st[(size_t)(R_LTIP + 3 * limb + 1) * N + env], st[(size_t)(R_LTIP + 3 * limb + 2) * N + env]);
  S.goal.w = st[(size_t)(R_GOAL + 0) * N + env]; S.goal.x = st[(size_t)(R_GOAL + 1) * N + env]; S.goal.y = st[(size_t)(R_GOAL + 2) * N + env]; S.goal.z = st[(size_t)(R_GOAL + 3) * N + env];
  S.succ = (int)cnt[0 * (size_t)N + env]; S.consec = (int)cnt[1 * (size_t)N + env]; S.greset = (int)cnt[2 * (size_t)N + env];
  S.reset = (int)cnt[3 * (size_t)N + env]; S.progress = (int)cnt[4 * (size_t)N + env]; int episode = (int)cnt[5 * (size_t)N + env];
  if (P->variant == 1) task_eval<MODE, 1>(P, limb, envl, I, S, O, sObs, sSt); else if (P->variant == 2) task_eval<MODE, 2>(P, limb, envl, I, S, O, sObs, sSt);
  else task_eval<MODE, 0>(P, limb, envl, I, S, O, sObs, sSt);
  if (active) {
    for (int a = 0; a < 3; a++) { st[(size_t)(R_LACT + jj[a]) * N + env] = S.lact[a]; st[(size_t)(R_LTGT + jj[a]) * N + env] = S.ltgt[a]; }
    if (limb == 0) st[(size_t)R_LRD * N + env] = S.lrd;
    st[(size_t)(R_LTIP + 3 * limb) * N + env] = S.ltip.x; st[(size_t)(R_LTIP + 3 * limb + 1) * N + env] = S.ltip.y; st[(size_t)(R_LTIP + 3 * limb + 2) * N + env] = S.ltip.z;
  }
  DrOut DO{};
  write_outputs<0>(P, A.W, N, env0, lane, limb, env, active, S, O, cnt, episode, sObs, sSt, DO);
}
__global__ void __launch_bounds__(64) k_task_eval(StepArgs A, const float* readback) {
  __shared__ __attribute__((aligned(16))) float sObs[ENVS_PER_WAVE * LM_MAX_OBS];
  __shared__ __attribute__((aligned(16))) float sSt[ENVS_PER_WAVE * 93];
  const lm_params* P = A.params + ((lm_block() * ENVS_PER_WAVE >= A.split) ? 1 : 0);
  if (P->mode == LM_MODE_LOCO) task_only_body<0>(A, P, readback, sObs, sSt); else task_only_body<1>(A, P, readback, sObs, sSt);
}

// ------------------------------------------------------------------------------------------------
// host side (C ABI)
// ------------------------------------------------------------------------------------------------
// public packed table -> the device layout of lm_dynamics.h (T_*: chain entries interleaved)
static void permute_table(const float* pub, float* dev) {
  memset(dev, 0, LM_ITAB_FLOATS * sizeof(float));
  {   // hub body: (m, com, I about COM) -> spatial inertia about the hub origin (m, h = m c, I_O [xx,yy,zz,xy,xz,yz]), constant in hub coordinates
    const double m = pub[0], c[3] = {pub[1], pub[2], pub[3]}, cc = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
    dev[0] = (float)m; dev[1] = (float)(m * c[0]); dev[2] = (float)(m * c[1]); dev[3] = (float)(m * c[2]);
    dev[4] = (float)(pub[4] + m * (cc - c[0] * c[0])); dev[5] = (float)(pub[5] + m * (cc - c[1] * c[1])); dev[6] = (float)(pub[6] + m * (cc - c[2] * c[2]));
    dev[7] = (float)(pub[7] - m * c[0] * c[1]); dev[8] = (float)(pub[8] - m * c[0] * c[2]); dev[9] = (float)(pub[9] - m * c[1] * c[2]);
  }
  for (int l = 0; l < 4; l++) {
    const float* s = pub + HUB_FLOATS + l * PUB_LIMB_STRIDE; float* d = dev + HUB_FLOATS + l * LIMB_STRIDE;
    for (int k = 0; k < 13; k++) { d[T_J0 + k] = s[k]; d[T_P1 + 2 * k] = s[13 + k]; d[T_P1 + 2 * k + 1] = s[39 + k]; d[T_P2 + 2 * k] = s[26 + k]; d[T_P2 + 2 * k + 1] = s[52 + k]; }
    for (int k = 0; k < 10; k++) { d[T_I0 + k] = s[65 + k]; d[T_Q1 + 2 * k] = s[75 + k]; d[T_Q1 + 2 * k + 1] = s[95 + k]; d[T_Q2 + 2 * k] = s[85 + k]; d[T_Q2 + 2 * k + 1] = s[105 + k]; }
    for (int k = 0; k < 7; k++) d[T_TIP + k] = s[115 + k];
  }
}

static thread_local char g_err[256] = "";
static int fail(int code, const char* msg) { snprintf(g_err, sizeof(g_err), "%s", msg); return code; }
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { snprintf(g_err, sizeof(g_err), "%s: %s", #x, hipGetErrorString(e_)); return LM_EHIP; } } while (0)

struct lm_engine {
  int N, n_tasks, split, nblocks, num_obs, device;
  int w2_min_envs;         // lm_step launches k_step_w2 (two wavefronts per SIMD) from this env count on; LM_W2_MIN_ENVS overrides 32769 (tests, A/B)
  int h2_max_envs;         // lm_step launches k_step_h2 (a helper wavefront per workgroup) up to this env count: while 2 wavefronts per 16 envs find a SIMD each
                           // (8192 envs on MI355X); LM_H2_MAX_ENVS overrides it (tests, A/B; 0 = never)
  int h3_max_envs;         // ... and k_step_h3 (two helper wavefronts per workgroup) up to this one: one workgroup per CU (4096 envs on MI355X: a wavefront of
                           // 466 registers has a SIMD to itself, so a second workgroup of three finds no room on a CU and waits for a second generation -
                           // measured at 5456 envs: 54.2 against k_step_h2's 31.7 us); LM_H3_MAX_ENVS overrides it; off when only LM_H2_MAX_ENVS is set (that forces k_step_h2 or k_step)
  uint32_t seed;
  lm_params* d_params;     // [2]
  float* d_table;
  float* d_state; int64_t* d_cnt; int64_t* d_drc; float* d_dr_phys; int dr_enabled;
  lm_reset_dr* d_reset_dr; // randomised engines: the reset-state channels of the two blocks, followed by float [LM_DR_RESET_ROWS][N] (LM_PTR_DR_RESET_STATE)
  lm_mass_dr* d_mass_dr;   // randomised engines: the mass channels of the two blocks, followed by float [LM_DR_MASS_ROWS][N] (LM_PTR_DR_MASS)
  lm_actuator_dr* d_actuator_dr;      // randomised engines: the actuator channels of the two blocks, followed by float [LM_DR_ACTUATOR_ROWS][N] (LM_PTR_DR_ACTUATOR)
  float h_body_mass[LM_NUM_BODIES];      // nominal body masses in table order (what lm_set_mass_randomization checks ranges against)
  float *d_obs, *d_states, *d_rew, *d_extras, *d_terms; long long* d_acc; int acc_rows;
  bool view_obs, view_states, view_terms;      // lm_ptr() handed out obs_buf / states_buf / the reward terms: lm_step keeps them current from then on
  float* d_contact;        // [LM_CONTACT_ROWS][N] contact record, allocated by the first lm_enable_contact_forces(h, 1) (LM_PTR_CONTACT)
  bool contact_on;         // lm_step / lm_substeps launch the *_cf kernels and write d_contact
  float* d_env_params;     // [LM_ENV_PARAM_ROWS][N] hold table followed by the row mask uint64 [2] (at env_mask_offset), allocated by lm_enable_env_params (LM_PTR_ENV_PARAMS);
                           // while it exists lm_step launches k_step_dr_hp / k_step_dr_pd_hp
  uint64_t env_mask[2];    // host copy of the row mask
  unsigned char mass_ch_on[2][LM_DR_MASS_CHANNELS], actuator_ch_on[2][LM_DR_ACTUATOR_CHANNELS];      // which mass / actuator channels the setters switched on, per block
  char* d_stats;           // int64 {num_successes, num_resets} x {all, first task, second task}; float success_rate x 3 at byte 48;
                           // uint32 count of contained blow-ups at byte 60
  lm_params h_params[2];
};

static void derive_params(lm_params* p) {
  // plate spatial inertia about its origin (plate coordinates) and its inverse (double precision Gauss-Jordan)
  double m = p->plate_mass, c[3] = {p->plate_com[0], p->plate_com[1], p->plate_com[2]};
  double cc = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
  double IO[3][3];
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) IO[i][j] = ((i == j) ? (p->plate_inertia[i] + m * cc) : 0.0) - m * c[i] * c[j];
  p->plate_si[0] = (float)m; p->plate_si[1] = (float)(m * c[0]); p->plate_si[2] = (float)(m * c[1]); p->plate_si[3] = (float)(m * c[2]);
  p->plate_si[4] = (float)IO[0][0]; p->plate_si[5] = (float)IO[1][1]; p->plate_si[6] = (float)IO[2][2];
  p->plate_si[7] = (float)IO[0][1]; p->plate_si[8] = (float)IO[0][2]; p->plate_si[9] = (float)IO[1][2];
  double h[3] = {m * c[0], m * c[1], m * c[2]};
  double hx[3][3] = {{0, -h[2], h[1]}, {h[2], 0, -h[0]}, {-h[1], h[0], 0}};
  double A[6][12];
  for (int i = 0; i < 6; i++) for (int j = 0; j < 12; j++) A[i][j] = (j - 6 == i) ? 1.0 : 0.0;
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { A[i][j] = IO[i][j]; A[i][3 + j] = hx[i][j]; A[3 + i][j] = -hx[i][j]; A[3 + i][3 + j] = (i == j) ? m : 0.0; }
  for (int col = 0; col < 6; col++) {
    int piv = col; for (int r = col + 1; r < 6; r++) if (fabs(A[r][col]) > fabs(A[piv][col])) piv = r;
    if (piv != col) for (int j = 0; j < 12; j++) { double t = A[col][j]; A[col][j] = A[piv][j]; A[piv][j] = t; }
    double d = A[col][col]; if (d == 0.0) d = 1e-30;
    for (int j = 0; j < 12; j++) A[col][j] /= d;
    for (int r = 0; r < 6; r++) if (r != col) { double f = A[r][col]; for (int j = 0; j < 12; j++) A[r][j] -= f * A[col][j]; }
  }
  for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) p->plate_phi[6 * i + j] = (float)A[i][6 + j];
  p->ctrl_dt_inv = (float)(1.0 / ((double)p->dt * (double)p->substeps));
  p->acc_dt_inv = (float)(1.0 / ((double)p->dt * (double)(p->acc_substeps > 0 ? p->acc_substeps : 1)));
}

// T [rows][N] on the host, zero except for what rule(e, col) writes for env e (col[r * N] = row r of that env), uploaded to dst
template <class T, class Rule> static bool upload_rows(T* dst, int rows, size_t N, Rule rule) {
  T* tmp = new T[(size_t)rows * N]();
  for (size_t e = 0; e < N; e++) rule(e, tmp + e);
  const hipError_t err = hipMemcpy(dst, tmp, (size_t)rows * N * sizeof(T), hipMemcpyHostToDevice);
  delete[] tmp; return err == hipSuccess;
}

// The engine's buffers belong to the device that was current in lm_create: a launch from a thread whose current
// device differs would run on the wrong GPU (multi-GPU hosts run one process per GPU, so this is a caller bug).
static bool on_device(const lm_engine* h) {
  int d = -1;
  return hipGetDevice(&d) == hipSuccess && d == h->device;
}
#define CHECK_DEVICE(h, fn) do { if (!on_device(h)) return fail(LM_EINVAL, fn ": the calling thread's current device is not the engine's device"); } while (0)

// ---- what the domain-randomisation families share on the host (lm_create's channel loops and the lm_set_*_randomization entry points)
static int fail_fn(int code, const char* fn, const char* msg) { snprintf(g_err, sizeof(g_err), "%s: %s", fn, msg); return code; }
// before a setter looks at a channel: arguments, a randomised engine (`record`: the family's device buffer), the block, the device
static int dr_set_entry(const char* fn, const lm_engine* h, const void* arg, const void* record, int block) {
  if (!h || !arg) return fail_fn(LM_EINVAL, fn, "null argument");
  if (!h->dr_enabled || !record) return fail_fn(LM_EINVAL, fn, "the engine was created without dr_enabled");
  if (block < 0 || block >= h->n_tasks) return fail_fn(LM_EINVAL, fn, "block must be 0 (or 1 on a two-task engine)");
  if (!on_device(h)) return fail_fn(LM_EINVAL, fn, "the calling thread's current device is not the engine's device");
  return LM_OK;
}
// operation and distribution in 0..2, interval not below `least` (0: on_reset / on_interval entries; LM_DR_ON_STARTUP: on_startup too)
static bool dr_channel_ok(const lm_dr_channel& ch, int least) {
  return ch.operation >= 0 && ch.operation <= 2 && ch.distribution >= 0 && ch.distribution <= 2 && ch.interval >= least;
}
// one (p0, p1) pair of a channel: finite, and positive where it bounds a log-uniform distribution.  NULL, or what is wrong with it
static const char* dr_pair_refusal(const lm_dr_channel& ch, float p0, float p1) {
  if (!std::isfinite(p0) || !std::isfinite(p1)) return "non-finite distribution parameters";
  if (ch.distribution == LM_DR_LOGUNIFORM && !(p0 > 0 && p1 > 0)) return "log-uniform bounds must be positive";
  return nullptr;
}

extern "C" {

const char* lm_last_error(void) { return g_err; }
const char* lm_version(void) { return "lm_engine 0.6 (gfx950, abi 5, policy tiles on the fp16 matrix pipe)"; }
int lm_abi_version(void) { return LM_ABI_VERSION; }

int lm_create(lm_engine** out, int n_envs, const float* table, const lm_params* params, int n_tasks, int split_env, uint32_t seed) {
  if (!out || !table || !params) return fail(LM_EINVAL, "lm_create: null argument");
  if (n_envs <= 0) return fail(LM_EINVAL, "lm_create: n_envs must be positive");
  if (n_envs >= (1 << (ACC_WIN_BITS - 1))) return fail(LM_EINVAL, "lm_create: n_envs must be below 2^25 per engine (width of the reset counts in the extras reduction)");
  if (n_tasks != 1 && n_tasks != 2) return fail(LM_EINVAL, "lm_create: n_tasks must be 1 or 2");
  // the stamp of the FIRST block is read before anything else of the struct: a caller built against another header passes a shifted layout
  if (params[0].abi_version != LM_ABI_VERSION || params[0].params_size != (int32_t)sizeof(lm_params) || params[0].table_floats != LM_TABLE_FLOATS)
    return fail(LM_EINVAL, "lm_create: ABI mismatch (lm_params.abi_version / params_size / table_floats differ from the library's LM_ABI_VERSION, sizeof(lm_params), LM_TABLE_FLOATS)");
  if (n_tasks == 2 && (params[1].abi_version != LM_ABI_VERSION || params[1].params_size != (int32_t)sizeof(lm_params) || params[1].table_floats != LM_TABLE_FLOATS))
    return fail(LM_EINVAL, "lm_create: ABI mismatch in the second parameter block");
  if (n_tasks == 2 && (split_env <= 0 || split_env >= n_envs || (split_env % ENVS_PER_WAVE) != 0))
    return fail(LM_EINVAL, "lm_create: split_env must be a multiple of 16 inside (0, n_envs)");
  for (int t = 0; t < n_tasks; t++) {
    const lm_params& p = params[t];
    if (!(p.dt > 0) || p.substeps <= 0 || p.pgs_iters < 0 || (p.mode != LM_MODE_LOCO && p.mode != LM_MODE_MANI))
      return fail(LM_EINVAL, "lm_create: invalid dt / substeps / pgs_iters / mode");
    if (p.pd_second_pass < 0 || p.pd_second_pass > 1) return fail(LM_EINVAL, "lm_create: pd_second_pass must be 0 or 1");
    if (p.drive_mode < 0 || p.drive_mode > 2 || (p.drive_mode != 0 && p.variant != 0) || (p.drive_mode == LM_DRIVE_POSITION && !(p.kd > 0)))
      return fail(LM_EINVAL, "lm_create: drive_mode must be 0 (velocity), 1 (position: kd > 0) or 2 (effort), and 0 for the PD-actuator variants");
    if ((p.num_obs != 64 && p.num_obs != LM_MAX_OBS) || p.num_obs != params[0].num_obs || p.variant < 0 || p.variant > 2 ||
        (p.variant == 1) != (p.num_obs == LM_MAX_OBS) || (p.variant >= 1 && !(p.kd > 0 && p.torque_div > 0 && p.acc_substeps >= 1 && p.acc_substeps <= p.substeps)))
      return fail(LM_EINVAL, "lm_create: invalid variant / num_obs (64 for velocity-drive and position-control tasks, 88 for custom-controller tasks, equal across tasks) or acc_substeps");
    if ((p.dr_enabled != 0) != (params[0].dr_enabled != 0)) return fail(LM_EINVAL, "lm_create: dr_enabled must be equal across tasks");
    if ((p.variant != 0) != (params[0].variant != 0)) return fail(LM_EINVAL, "lm_create: both parameter blocks must be of one actuator family (velocity drive: variant 0; PD actuator: variants 1 / 2)");
    if (p.dr_enabled) for (int c = 0; c < LM_DR_CHANNELS; c++) {
      const lm_dr_channel& ch = p.dr[c];
      if (!ch.enabled) continue;
      const bool noise_reset = (c == LM_DR_OBS_RESET || c == LM_DR_ACT_RESET), noise_interval = (c == LM_DR_OBS_INTERVAL || c == LM_DR_ACT_INTERVAL);
      if (!dr_channel_ok(ch, 0) || (noise_reset && ch.interval != 0) || (noise_interval && ch.interval < 1) || ((noise_reset || noise_interval) && ch.operation == LM_DR_DIRECT) ||
          (ch.distribution == LM_DR_LOGUNIFORM && !(ch.p0[0] > 0 && ch.p1[0] > 0)) || p.dr_min_frequency < 0)
        return fail(LM_EINVAL, "lm_create: invalid domain-randomisation channel (operation / distribution / interval / parameters)");
    }
    for (int c = 0; c < LM_DR_MATERIALS; c++) {
      const lm_dr_channel& ch = p.dr_mat[c];
      if (!ch.enabled) continue;
      if (!p.dr_enabled || !dr_channel_ok(ch, LM_DR_ON_STARTUP) || p.dr_mat_buckets[c] < 0 || (ch.distribution == LM_DR_LOGUNIFORM && !(ch.p0[1] > 0 && ch.p1[1] > 0)) ||
          (c == LM_DR_MAT_OTHER && p.mode != LM_MODE_MANI))
        return fail(LM_EINVAL, "lm_create: invalid contact-material channel (needs dr_enabled; operation / distribution / interval / num_buckets / "
                               "parameters; the plate channel only on a manipulation block)");
    }
    if ((p.dr_mat[0].enabled || p.dr_mat[1].enabled) && (p.friction_combine < 0 || p.friction_combine > 3 || !(p.friction_scale >= 0.f)))
      return fail(LM_EINVAL, "lm_create: friction_combine must be 0..3 and friction_scale >= 0 with a contact-material channel");
  }
  int device = 0;
  HIPCHK(hipGetDevice(&device));
  lm_engine* h = new (std::nothrow) lm_engine();
  if (!h) return fail(LM_ENOMEM, "lm_create: host allocation failed");
  memset(h, 0, sizeof(*h));
  h->device = device;          // every buffer lives on the device current at creation; launches check it (on_device)
  h->N = n_envs; h->n_tasks = n_tasks; h->split = (n_tasks == 2) ? split_env : n_envs; h->seed = seed;
  h->nblocks = (n_envs + ENVS_PER_WAVE - 1) / ENVS_PER_WAVE;
  { const char* e = getenv("LM_W2_MIN_ENVS"); h->w2_min_envs = e ? atoi(e) : 32769; }
  {
    // beyond one wavefront per SIMD a 128-thread workgroup costs a second generation of wavefronts: k_step / k_step_w2 from there on
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) cus = 0;
    h->h2_max_envs = (4 * cus / 2) * ENVS_PER_WAVE;
    if (const char* e = getenv("LM_H2_MAX_ENVS")) {      // a malformed or negative value is ignored
      char* end = nullptr; const long v = strtol(e, &end, 10);
      if (end != e && *end == '\0' && v >= 0 && v <= INT32_MAX) h->h2_max_envs = (int)v;
    }
    h->h3_max_envs = getenv("LM_H2_MAX_ENVS") ? 0 : cus * ENVS_PER_WAVE;
    if (const char* e = getenv("LM_H3_MAX_ENVS")) {      // a malformed or negative value is ignored
      char* end = nullptr; const long v = strtol(e, &end, 10);
      if (end != e && *end == '\0' && v >= 0 && v <= INT32_MAX) h->h3_max_envs = (int)v;
    }
  }
  h->num_obs = params[0].num_obs; h->dr_enabled = params[0].dr_enabled != 0;
  h->h_params[0] = params[0]; h->h_params[1] = params[n_tasks - 1];
  derive_params(&h->h_params[0]); derive_params(&h->h_params[1]);
  size_t N = (size_t)n_envs;
#define ALLOC(ptr, bytes) do { hipError_t e_ = hipMalloc((void**)&(ptr), (bytes)); if (e_ != hipSuccess) { snprintf(g_err, sizeof(g_err), "hipMalloc(%zu): %s", (size_t)(bytes), hipGetErrorString(e_)); lm_destroy(h); return LM_EHIP; } \
    e_ = hipMemset((ptr), 0, (bytes)); if (e_ != hipSuccess) { snprintf(g_err, sizeof(g_err), "hipMemset: %s", hipGetErrorString(e_)); lm_destroy(h); return LM_EHIP; } } while (0)
  ALLOC(h->d_params, 2 * sizeof(lm_params));
  ALLOC(h->d_table, LM_ITAB_FLOATS * sizeof(float));
  ALLOC(h->d_state, LM_STATE_ROWS * N * sizeof(float));
  ALLOC(h->d_cnt, LM_CNT_ROWS * N * sizeof(int64_t));
  ALLOC(h->d_drc, LM_DR_CNT_ROWS * N * sizeof(int64_t));
  ALLOC(h->d_dr_phys, LM_DR_PHYS_ROWS * N * sizeof(float));
  if (h->dr_enabled) ALLOC(h->d_reset_dr, 2 * sizeof(lm_reset_dr) + LM_DR_RESET_ROWS * N * sizeof(float));      // zeros: all four channels off
  if (h->dr_enabled) ALLOC(h->d_mass_dr, 2 * sizeof(lm_mass_dr) + LM_DR_MASS_ROWS * N * sizeof(float));         // zeros: all three channels off
  if (h->dr_enabled) ALLOC(h->d_actuator_dr, 2 * sizeof(lm_actuator_dr) + LM_DR_ACTUATOR_ROWS * N * sizeof(float));      // zeros: all three channels off
  ALLOC(h->d_obs, N * (size_t)h->num_obs * sizeof(float));
  ALLOC(h->d_states, N * 93 * sizeof(float));
  ALLOC(h->d_rew, N * sizeof(float));
  ALLOC(h->d_extras, 16 * sizeof(float));
  ALLOC(h->d_terms, LM_TERM_ROWS * N * sizeof(float));
  h->acc_rows = LM_ACC_COPIES;      // a counted accumulator word takes at most 4095 arrivals (write_outputs)
  while (((N + ENVS_PER_WAVE - 1) / ENVS_PER_WAVE + h->acc_rows - 1) / h->acc_rows > (int)ACC_CNT_MASK) h->acc_rows *= 2;
  ALLOC(h->d_acc, (16 + (size_t)h->acc_rows * 16) * sizeof(long long));      // row 0: totals of a launch; rows 1..: first-level rows
  ALLOC(h->d_stats, 64);
#undef ALLOC
  float itab[LM_ITAB_FLOATS]; permute_table(table, itab);      // public packed layout -> the device's chain-interleaved layout
  if (hipMemcpy(h->d_params, h->h_params, 2 * sizeof(lm_params), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->d_table, itab, LM_ITAB_FLOATS * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
    lm_destroy(h); return fail(LM_EHIP, "lm_create: parameter / table upload failed");
  }
  h->h_body_mass[0] = itab[0];
  for (int l = 0; l < 4; l++) {
    const float* d = itab + HUB_FLOATS + l * LIMB_STRIDE; float* m = h->h_body_mass + 1 + 5 * l;
    m[0] = d[T_I0]; m[1] = d[T_Q1]; m[2] = d[T_Q2]; m[3] = d[T_Q1 + 1]; m[4] = d[T_Q2 + 1];      // shell, link4, link3, link1, link2
  }
  const auto block_of = [&](size_t e) -> const lm_params& { return h->h_params[(int)e >= h->split ? 1 : 0]; };
  bool up = true;
  // the mass and actuator records start at the nominal values (a step rewrites only the rows of the channels that are on): plate mass, inertia
  // factor 1, body masses; the blocks' gains, no latency
  if (h->d_mass_dr) up = upload_rows((float*)(h->d_mass_dr + 2), LM_DR_MASS_ROWS, N, [&](size_t e, float* col) {
    col[0] = block_of(e).plate_mass; col[N] = 1.f;
    for (int b = 0; b < LM_NUM_BODIES; b++) col[(size_t)(2 + b) * N] = h->h_body_mass[b]; });
  if (h->d_actuator_dr) up = up && upload_rows((float*)(h->d_actuator_dr + 2), LM_DR_ACTUATOR_ROWS, N, [&](size_t e, float* col) { col[0] = block_of(e).pd_kp; col[N] = block_of(e).kd; });
  // identity quaternions so that an un-reset state is still valid; reset_buf = 1 (rl_task.py:111)
  up = up && upload_rows(h->d_state, LM_STATE_ROWS, N, [&](size_t, float* col) { col[(size_t)(R_FB0 + 3) * N] = 1.f; col[(size_t)(R_FB1 + 3) * N] = 1.f; col[(size_t)R_GOAL * N] = 1.f; });
  up = up && upload_rows(h->d_cnt, LM_CNT_ROWS, N, [&](size_t, int64_t* col) { col[3 * N] = 1; });
  if (!up) { lm_destroy(h); return fail(LM_EHIP, "lm_create: initial upload failed"); }
  *out = h;
  return LM_OK;
}

int lm_destroy(lm_engine* h) {
  if (!h) return LM_OK;
  void* ptrs[] = {h->d_params, h->d_table, h->d_state, h->d_cnt, h->d_drc, h->d_dr_phys, h->d_reset_dr, h->d_mass_dr, h->d_actuator_dr, h->d_obs, h->d_states, h->d_rew, h->d_extras, h->d_terms, h->d_acc, h->d_stats, h->d_contact, h->d_env_params};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  delete h;
  return LM_OK;
}

// the row mask of the hold table sits behind its LM_ENV_PARAM_ROWS x N floats, at the next 8-byte boundary (N may be odd)
static size_t env_mask_offset(int N) { return ((size_t)LM_ENV_PARAM_ROWS * (size_t)N + 1) & ~(size_t)1; }

// the step kernels' kind of parameter block t: actuator family x task mode (StepArgs::kind, lm_step.h)
static int block_kind(const lm_engine* h, int t) { return h->h_params[t].variant * 2 + (h->h_params[t].mode == LM_MODE_MANI ? 1 : 0); }

static StepArgs make_args(lm_engine* h, const float* actions, const float* goal_rand, float* out_obs, float* out_states, float* out_rew, int64_t* out_resets) {
  StepArgs A;
  A.params = h->d_params; A.table = h->d_table; A.state = h->d_state; A.cnt = h->d_cnt; A.actions = actions; A.goal_rand = goal_rand;
  A.W.obs_buf = h->d_obs; A.W.states_buf = h->d_states; A.W.rew_buf = h->d_rew; A.W.terms = h->d_terms; A.W.acc = h->d_acc;
  // first block of the second task: rounded up, so that the ragged last block of a single-task engine (split = N) counts into the first-task
  // window like every other one (the halves of joint_locomanipulation.py:846-859; a two-task split is a multiple of 16, lm_create)
  A.W.stats = (char*)h->d_stats; A.W.extras = h->d_extras; A.W.out_extras = nullptr; A.W.split_block = (h->split + ENVS_PER_WAVE - 1) / ENVS_PER_WAVE; A.W.acc_rows = h->acc_rows;
  A.W.out_obs = out_obs; A.W.out_states = out_states; A.W.out_rew = out_rew; A.W.out_resets = out_resets;
  A.N = h->N; A.split = h->split; A.seed = h->seed; A.skip_reset = 0; A.nsub = -1; A.drc = h->d_drc; A.dr_phys = h->d_dr_phys; A.reset_dr = h->d_reset_dr; A.mass_dr = h->d_mass_dr;
  A.env_params = h->d_env_params; A.contact = h->contact_on ? h->d_contact : nullptr; A.actuator_dr = h->d_actuator_dr;
  A.env_mask = h->d_env_params ? (const uint64_t*)(h->d_env_params + env_mask_offset(h->N)) : nullptr;
  for (int t = 0; t < 2; t++) A.kind[t] = block_kind(h, t);
  return A;
}

// The engine's own unclipped buffers (task.obs_buf / states_buf, rl_task.py:104-113, and the per-env reward terms) are a second copy of
// what the caller's out_obs / out_states receive clipped: a step writes them only once somebody has asked lm_ptr() for them (the Python
// task does, at construction), or when the caller passes no output buffer of that kind.  628 + 44 B per env-step of stores otherwise.
static void drop_unrequested_views(const lm_engine* h, StepArgs& A) {
  if (!h->view_obs && A.W.out_obs) A.W.obs_buf = nullptr;
  if (!h->view_states && A.W.out_states) A.W.states_buf = nullptr;
  if (!h->view_terms) A.W.terms = nullptr;
}

#ifdef LM_STAMPS
extern "C" int lm_debug_stamps(unsigned long long* out) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(lm_stamp_out), sizeof(lm_stamp_out)) == hipSuccess ? 0 : -1; }
#endif

// Which velocity-drive kernel lm_step launches on an engine without randomisation and contact reporting: 0 = k_step (one wavefront per 16 envs),
// 1 = k_step_w2 (two such workgroups per SIMD: locomotion-only engines from w2_min_envs on), 2 = k_step_h2 (a helper wavefront beside each:
// engines with a locomotion block up to h2_max_envs), 3 = k_step_h3 (two helper wavefronts: the same engines up to h3_max_envs).  Every other
// engine: 0, the one-wavefront kernel of its family.
static int step_variant(const lm_engine* h) {
  const int k0 = block_kind(h, 0), k1 = block_kind(h, 1);
  if (h->contact_on || h->dr_enabled || k0 >= 2 || k1 >= 2) return 0;
  if (k0 == 0 && k1 == 0 && h->N >= h->w2_min_envs) return 1;
  if ((k0 == 0 || k1 == 0) && h->N <= h->h3_max_envs) return 3;
  if ((k0 == 0 || k1 == 0) && h->N <= h->h2_max_envs) return 2;
  return 0;
}
// (not part of the C ABI: for tests and A/B runs that must know which kernel ran; -1 without an engine)
int lm_internal_step_variant(const lm_engine* h) { return h ? step_variant(h) : -1; }

int lm_step(lm_engine* h, const float* actions, const float* goal_rand, float* out_obs, float* out_states, float* out_rew,
            int64_t* out_resets, float* out_extras, void* stream) {
  if (!h || !actions) return fail(LM_EINVAL, "lm_step: null handle or actions");
  CHECK_DEVICE(h, "lm_step");
  hipStream_t s = (hipStream_t)stream;
  StepArgs A = make_args(h, actions, goal_rand, out_obs, out_states, out_rew, out_resets); A.W.out_extras = out_extras;
  drop_unrequested_views(h, A);
  const bool pd = A.kind[0] >= 2;                                  // both blocks are of one actuator family (lm_create)
  const int variant = step_variant(h);
  if (variant == 1) lm_internal_launch_step_w2(&A, h->nblocks, s);      // locomotion, two wavefronts per SIMD: ahead beyond 32 768 envs
  else if (variant == 3) lm_internal_launch_step_h3(&A, h->nblocks, s);      // two helper wavefronts per workgroup: ahead up to one workgroup per CU
  else if (variant == 2) lm_internal_launch_step_h2(&A, h->nblocks, s);      // a helper wavefront per workgroup: ahead while half the SIMDs are idle
  else if (h->d_env_params) lm_internal_launch_step_hp(&A, pd ? 1 : 0, h->nblocks, s);      // caller-held per-env parameters: the randomised kernels with the hold (never with reporting)
  else {
    void (*kern)(StepArgs) = h->contact_on ? (h->dr_enabled ? (pd ? k_step_dr_pd_cf : k_step_dr_cf) : (pd ? k_step_pd_cf : k_step_cf))      // with reporting: one-wavefront kernels at every size
                                           : (h->dr_enabled ? (pd ? k_step_dr_pd : k_step_dr) : (pd ? k_step_pd : k_step));
    hipLaunchKernelGGL(kern, dim3(h->nblocks), dim3(64), 0, s, A);
  }
  HIPCHK(hipGetLastError());
  return LM_OK;
}

int lm_post_physics(lm_engine* h, const float* actions, float* out_obs, float* out_states, float* out_rew,
                    int64_t* out_resets, float* out_extras, void* stream) {
  if (!h || !actions) return fail(LM_EINVAL, "lm_post_physics: null handle or actions");
  CHECK_DEVICE(h, "lm_post_physics");
  if (h->dr_enabled) return fail(LM_EINVAL, "lm_post_physics: a randomised engine runs through lm_step only");
  hipStream_t s = (hipStream_t)stream;
  StepArgs A = make_args(h, actions, nullptr, out_obs, out_states, out_rew, out_resets); A.W.out_extras = out_extras;
  A.skip_reset = 1; A.nsub = 0;
  void (*kern)(StepArgs) = A.kind[0] >= 2 ? k_step_pd : k_step;
  hipLaunchKernelGGL(kern, dim3(h->nblocks), dim3(64), 0, s, A);
  HIPCHK(hipGetLastError());
  return LM_OK;
}

int lm_set_reset_randomization(lm_engine* h, int block, const lm_reset_dr* rd) {
  const char* const fn = "lm_set_reset_randomization";
  if (int rc = dr_set_entry(fn, h, rd, h ? h->d_reset_dr : nullptr, block)) return rc;
  for (int c = 0; c < LM_DR_RESET_CHANNELS; c++) {
    const lm_dr_channel& ch = rd->ch[c];
    if (!ch.enabled) continue;
    const int ncomp = (c == LM_DR_RESET_POSITION || c == LM_DR_RESET_ORIENTATION) ? 3 : 1;      // the joint channels read p0[0] / p1[0]
    if (!dr_channel_ok(ch, INT32_MIN)) return fail_fn(LM_EINVAL, fn, "invalid operation / distribution");      // the interval has a refusal of its own
    if (ch.interval != 0) return fail_fn(LM_EINVAL, fn, "the reset-state channels are on_reset entries (interval 0)");
    if (ch.operation == LM_DR_SCALING && (c == LM_DR_RESET_JOINT_VEL || c == LM_DR_RESET_ORIENTATION))
      return fail_fn(LM_EINVAL, fn, "scaling makes no sense on the joint velocities (nominal 0) or on the orientation (a quaternion)");
    for (int k = 0; k < ncomp; k++)
      if (const char* why = dr_pair_refusal(ch, ch.p0[k], ch.p1[k])) return fail_fn(LM_EINVAL, fn, why);
  }
  HIPCHK(hipMemcpy(h->d_reset_dr + block, rd, sizeof(lm_reset_dr), hipMemcpyHostToDevice));
  return LM_OK;
}

// least mass (or density factor) a bounded distribution can produce from `nominal`: <= 0 is refused
static bool mass_range_ok(const lm_dr_channel& ch, float p0, float p1, float nominal) {
  if (ch.distribution == LM_DR_GAUSSIAN) return true;      // unbounded: the floor takes the tail
  const float lo = p0 < p1 ? p0 : p1;
  const float least = ch.operation == LM_DR_ADDITIVE ? nominal + lo : ch.operation == LM_DR_SCALING ? nominal * lo : lo;
  return least > 0.f;
}
int lm_set_mass_randomization(lm_engine* h, int block, const lm_mass_dr* md) {
  const char* const fn = "lm_set_mass_randomization";
  if (int rc = dr_set_entry(fn, h, md, h ? h->d_mass_dr : nullptr, block)) return rc;
  const lm_params& P = h->h_params[block];
  float s_least = 1.f;      // least density factor: the nominal of the plate-mass channel is s x plate_mass
  for (int c = 0; c < LM_DR_MASS_CHANNELS; c++) {
    const lm_dr_channel& ch = md->ch[c == 0 ? LM_DR_MASS_PLATE_DENSITY : c == 1 ? LM_DR_MASS_PLATE : LM_DR_MASS_BODIES];      // density first
    const int kind = (int)(&ch - md->ch);
    if (!ch.enabled) continue;
    if (!dr_channel_ok(ch, LM_DR_ON_STARTUP)) return fail_fn(LM_EINVAL, fn, "invalid operation / distribution / interval");
    if (kind != LM_DR_MASS_BODIES && P.mode != LM_MODE_MANI) return fail_fn(LM_EINVAL, fn, "the plate channels exist on manipulation blocks only");
    if (kind == LM_DR_MASS_PLATE_DENSITY && (ch.interval != LM_DR_ON_STARTUP || ch.operation != LM_DR_SCALING))
      return fail_fn(LM_EINVAL, fn, "the density channel is on_startup + scaling only (no nominal density exists: the URDF gives mass and inertia, no volume)");
    const int n = kind == LM_DR_MASS_BODIES ? LM_NUM_BODIES : 1;
    for (int k = 0; k < n; k++) {
      const float p0 = kind == LM_DR_MASS_BODIES ? md->body_p0[k] : ch.p0[0], p1 = kind == LM_DR_MASS_BODIES ? md->body_p1[k] : ch.p1[0];
      if (const char* why = dr_pair_refusal(ch, p0, p1)) return fail_fn(LM_EINVAL, fn, why);
      const float nominal = kind == LM_DR_MASS_BODIES ? h->h_body_mass[k] : kind == LM_DR_MASS_PLATE ? s_least * P.plate_mass : 1.f;
      if (!mass_range_ok(ch, p0, p1, nominal)) return fail_fn(LM_EINVAL, fn, "the distribution's range reaches a non-positive mass");
      if (kind == LM_DR_MASS_PLATE_DENSITY) s_least = ch.distribution == LM_DR_GAUSSIAN ? LM_DR_MASS_FLOOR : (p0 < p1 ? p0 : p1);
    }
  }
  HIPCHK(hipMemcpy(h->d_mass_dr + block, md, sizeof(lm_mass_dr), hipMemcpyHostToDevice));
  for (int c = 0; c < LM_DR_MASS_CHANNELS; c++) h->mass_ch_on[block][c] = md->ch[c].enabled != 0;
  return LM_OK;
}

int lm_set_actuator_randomization(lm_engine* h, int block, const lm_actuator_dr* ad) {
  const char* const fn = "lm_set_actuator_randomization";
  if (int rc = dr_set_entry(fn, h, ad, h ? h->d_actuator_dr : nullptr, block)) return rc;
  const lm_params& P = h->h_params[block];
  for (int c = 0; c < LM_DR_ACTUATOR_CHANNELS; c++) {
    const lm_dr_channel& ch = ad->ch[c];
    if (!ch.enabled) continue;
    if (!dr_channel_ok(ch, LM_DR_ON_STARTUP)) return fail_fn(LM_EINVAL, fn, "invalid operation / distribution / interval");
    if (c == LM_DR_ACTUATOR_KP && P.variant == 0 && P.drive_mode != LM_DRIVE_POSITION)
      return fail_fn(LM_EINVAL, fn, "the kp channel needs a position gain (variants 1 / 2, or variant 0 in position drive mode)");
    if (c == LM_DR_ACTUATOR_KD && P.variant == 0 && P.drive_mode == LM_DRIVE_EFFORT)
      return fail_fn(LM_EINVAL, fn, "the kd channel has nothing to act on in effort drive mode (gains off)");
    if (c == LM_DR_ACTUATOR_LATENCY && P.variant == 0)
      return fail_fn(LM_EINVAL, fn, "the latency channel exists on the PD-actuator variants (1 / 2) only");
    if (c == LM_DR_ACTUATOR_LATENCY && ch.operation == LM_DR_SCALING)
      return fail_fn(LM_EINVAL, fn, "scaling the command latency is refused (its nominal is 0)");
    if (const char* why = dr_pair_refusal(ch, ch.p0[0], ch.p1[0])) return fail_fn(LM_EINVAL, fn, why);
    if (c != LM_DR_ACTUATOR_LATENCY && !mass_range_ok(ch, ch.p0[0], ch.p1[0], c == LM_DR_ACTUATOR_KP ? P.pd_kp : P.kd))
      return fail_fn(LM_EINVAL, fn, "the distribution's range reaches a non-positive gain");
  }
  HIPCHK(hipMemcpy(h->d_actuator_dr + block, ad, sizeof(lm_actuator_dr), hipMemcpyHostToDevice));
  for (int c = 0; c < LM_DR_ACTUATOR_CHANNELS; c++) h->actuator_ch_on[block][c] = ad->ch[c].enabled != 0;
  return LM_OK;
}

int lm_enable_contact_forces(lm_engine* h, int on) {
  if (!h) return fail(LM_EINVAL, "lm_enable_contact_forces: null handle");
  CHECK_DEVICE(h, "lm_enable_contact_forces");
  if (on && h->d_env_params) return fail(LM_EINVAL, "lm_enable_contact_forces: the engine holds per-env parameters (lm_enable_env_params); the two do not combine yet");
  if (on && !h->d_contact) {
    const size_t row = (size_t)h->N * sizeof(float), bytes = LM_CONTACT_ROWS * row;
    float* p = nullptr;
    HIPCHK(hipMalloc((void**)&p, bytes + row));      // one guard row behind the record: all bits set, written by no kernel (the tests read it)
    if (hipMemset(p, 0, bytes) != hipSuccess || hipMemset((char*)p + bytes, 0xFF, row) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { (void)hipFree(p); return fail(LM_EHIP, "lm_enable_contact_forces: clearing the record failed"); }
    h->d_contact = p;
  }
  h->contact_on = on != 0;
  return LM_OK;
}

// ---- per-env parameters held by the caller (include/lm_engine.h, LM_ENV_PARAM_ROWS)
enum { HP_MASS0 = LM_DR_PHYS_ROWS, HP_ACT0 = LM_DR_PHYS_ROWS + LM_DR_MASS_ROWS };      // first rows of the mass and the actuator part
static int env_params_entry(const char* fn, const lm_engine* h, int row0, int nrows) {
  if (!h) return fail_fn(LM_EINVAL, fn, "null handle");
  if (!on_device(h)) return fail_fn(LM_EINVAL, fn, "the calling thread's current device is not the engine's device");
  if (!h->d_env_params) return fail_fn(LM_EINVAL, fn, "env params are not enabled on this engine (lm_enable_env_params)");
  if (row0 < 0 || nrows <= 0 || row0 > LM_ENV_PARAM_ROWS - nrows) return fail_fn(LM_EINVAL, fn, "rows outside [0, LM_ENV_PARAM_ROWS)");
  return LM_OK;
}
static int env_mask_upload(lm_engine* h) {
  HIPCHK(hipMemcpy(h->d_env_params + env_mask_offset(h->N), h->env_mask, sizeof(h->env_mask), hipMemcpyHostToDevice));
  return LM_OK;
}
// NULL when some block of the engine reads row r, or why none does (the reasons of lm_set_actuator_randomization / lm_set_mass_randomization)
static const char* env_row_refusal(const lm_engine* h, int r) {
  bool mani = false, kp = false, kd = false, pdv = false;
  for (int b = 0; b < h->n_tasks; b++) {
    const lm_params& P = h->h_params[b];
    mani |= P.mode == LM_MODE_MANI; pdv |= P.variant != 0;
    kp |= P.variant != 0 || P.drive_mode == LM_DRIVE_POSITION; kd |= P.variant != 0 || P.drive_mode != LM_DRIVE_EFFORT;
  }
  if ((r == HP_MASS0 || r == HP_MASS0 + 1) && !mani) return "the plate rows exist on engines with a manipulation block only";
  if (r == HP_ACT0 + LM_DR_ACTUATOR_KP && !kp) return "the kp row needs a position gain (variants 1 / 2, or variant 0 in position drive mode)";
  if (r == HP_ACT0 + LM_DR_ACTUATOR_KD && !kd) return "the kd row has nothing to act on in effort drive mode (gains off)";
  if (r == HP_ACT0 + LM_DR_ACTUATOR_LATENCY && !pdv) return "the latency row exists on the PD-actuator variants (1 / 2) only";
  return nullptr;
}
// NULL when `v` may be held in row r for env e, or what is wrong with it
static const char* env_value_refusal(const lm_engine* h, int r, size_t e, float v) {
  if (!std::isfinite(v)) return "non-finite value";
  if (r >= HP_MASS0 && r < HP_ACT0 + LM_DR_ACTUATOR_LATENCY) return v > 0.f ? nullptr : "masses, the plate's inertia factor, kp and kd must be positive";
  if (r == HP_ACT0 + LM_DR_ACTUATOR_LATENCY) {
    const lm_params& P = h->h_params[(int)e >= h->split ? 1 : 0];
    if (v != floorf(v) || v < 0.f || (P.variant != 0 && v > (float)P.substeps)) return "the latency must be a whole number of sub-steps in [0, substeps]";
    return nullptr;
  }
  if (r >= 24 && r < 30) return nullptr;      // gravity and the base-link force: any finite vector
  return v >= 0.f ? nullptr : "mu, max efforts, max joint velocities and joint damping must not be negative";
}
// mass / actuator row r: is it written by a channel of block b, and its nominal value there (what the record shows until a channel draws)
static bool env_row_has_channel(const lm_engine* h, int r, int b) {
  if (r == HP_MASS0) return h->mass_ch_on[b][LM_DR_MASS_PLATE] || h->mass_ch_on[b][LM_DR_MASS_PLATE_DENSITY];
  if (r == HP_MASS0 + 1) return h->mass_ch_on[b][LM_DR_MASS_PLATE] || h->mass_ch_on[b][LM_DR_MASS_PLATE_DENSITY];
  if (r < HP_ACT0) return h->mass_ch_on[b][LM_DR_MASS_BODIES];
  if (r < HP_ACT0 + LM_DR_ACTUATOR_LATENCY) return h->actuator_ch_on[b][LM_DR_ACTUATOR_KP] || h->actuator_ch_on[b][LM_DR_ACTUATOR_KD];
  return h->actuator_ch_on[b][LM_DR_ACTUATOR_LATENCY];
}
static float env_row_nominal(const lm_engine* h, int r, int b) {
  const lm_params& P = h->h_params[b];
  if (r == HP_MASS0) return P.plate_mass;
  if (r == HP_MASS0 + 1) return 1.f;
  if (r < HP_ACT0) return h->h_body_mass[r - HP_MASS0 - 2];
  return r == HP_ACT0 ? P.pd_kp : r == HP_ACT0 + 1 ? P.kd : 0.f;
}

int lm_enable_env_params(lm_engine* h) {
  const char* const fn = "lm_enable_env_params";
  if (!h) return fail_fn(LM_EINVAL, fn, "null handle");
  if (!on_device(h)) return fail_fn(LM_EINVAL, fn, "the calling thread's current device is not the engine's device");
  if (!h->dr_enabled) return fail_fn(LM_EINVAL, fn, "the engine was created without dr_enabled (the un-randomised kernels carry no per-env parameters)");
  if (h->contact_on) return fail_fn(LM_EINVAL, fn, "contact-force reporting is on (lm_enable_contact_forces); the two do not combine yet");
  if (h->d_env_params) return LM_OK;
  const size_t bytes = env_mask_offset(h->N) * sizeof(float) + sizeof(h->env_mask);
  float* p = nullptr;
  HIPCHK(hipMalloc((void**)&p, bytes));
  if (hipMemset(p, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { (void)hipFree(p); return fail(LM_EHIP, "lm_enable_env_params: clearing the table failed"); }
  h->env_mask[0] = h->env_mask[1] = 0; h->d_env_params = p;
  return LM_OK;
}

int lm_set_env_params(lm_engine* h, int row0, int nrows, const float* values_host) {
  const char* const fn = "lm_set_env_params";
  if (int rc = env_params_entry(fn, h, row0, nrows)) return rc;
  if (!values_host) return fail_fn(LM_EINVAL, fn, "null values");
  const size_t N = (size_t)h->N;
  for (int r = row0; r < row0 + nrows; r++) {      // everything is checked before anything is copied
    if (const char* why = env_row_refusal(h, r)) return fail_fn(LM_EINVAL, fn, why);
    const float* row = values_host + (size_t)(r - row0) * N;
    for (size_t e = 0; e < N; e++)
      if (const char* why = env_value_refusal(h, r, e, row[e])) return fail_fn(LM_EINVAL, fn, why);
  }
  // every step enqueued before this call, on whichever stream, runs with the rows as they were: a blocking copy alone is ordered against the
  // null stream only, and would overtake work queued on a caller's non-blocking stream
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(h->d_env_params + (size_t)row0 * N, values_host, (size_t)nrows * N * sizeof(float), hipMemcpyHostToDevice));
  for (int r = row0; r < row0 + nrows; r++) h->env_mask[r >> 6] |= 1ull << (r & 63);
  return env_mask_upload(h);
}

int lm_clear_env_params(lm_engine* h, int row0, int nrows) {
  const char* const fn = "lm_clear_env_params";
  if (int rc = env_params_entry(fn, h, row0, nrows)) return rc;
  const size_t N = (size_t)h->N;
  HIPCHK(hipDeviceSynchronize());      // as in lm_set_env_params: the mask and the record rows below are read by steps that may still be queued
  for (int r = row0; r < row0 + nrows; r++) {
    if (!((h->env_mask[r >> 6] >> (r & 63)) & 1ull)) continue;
    h->env_mask[r >> 6] &= ~(1ull << (r & 63));
    if (r < HP_MASS0) continue;      // LM_PTR_DR_PHYS is rewritten by every step
    // a mass / actuator record row is written only while a channel or a hold of its group is on: where no channel writes it, it shows the nominal value again
    float* rec = r < HP_ACT0 ? (float*)(h->d_mass_dr + 2) + (size_t)(r - HP_MASS0) * N : (float*)(h->d_actuator_dr + 2) + (size_t)(r - HP_ACT0) * N;
    float* tmp = new (std::nothrow) float[N];
    if (!tmp) return fail(LM_ENOMEM, "lm_clear_env_params: host allocation failed");
    hipError_t err = hipMemcpy(tmp, rec, N * sizeof(float), hipMemcpyDeviceToHost);
    for (size_t e = 0; e < N && err == hipSuccess; e++) { const int b = (int)e >= h->split ? 1 : 0; if (!env_row_has_channel(h, r, b)) tmp[e] = env_row_nominal(h, r, b); }
    if (err == hipSuccess) err = hipMemcpy(rec, tmp, N * sizeof(float), hipMemcpyHostToDevice);
    delete[] tmp;
    if (err != hipSuccess) return fail(LM_EHIP, "lm_clear_env_params: restoring a record row failed");
  }
  return env_mask_upload(h);
}

int lm_env_params_held(const lm_engine* h, uint64_t* mask_out) {
  if (!h || !mask_out) return fail(LM_EINVAL, "lm_env_params_held: null argument");
  if (!h->d_env_params) return fail(LM_EINVAL, "lm_env_params_held: env params are not enabled on this engine (lm_enable_env_params)");
  mask_out[0] = h->env_mask[0]; mask_out[1] = h->env_mask[1];
  return LM_OK;
}

int lm_reset_all(lm_engine* h, void* stream) {
  if (!h) return fail(LM_EINVAL, "lm_reset_all: null handle");
  CHECK_DEVICE(h, "lm_reset_all");
  hipLaunchKernelGGL(k_reset_all, dim3((h->N + 63) / 64), dim3(64), 0, (hipStream_t)stream, h->d_cnt, h->N);
  HIPCHK(hipGetLastError());
  return LM_OK;
}

int lm_task_eval(lm_engine* h, const float* readback, const float* actions, float* out_obs, float* out_states, float* out_rew,
                 int64_t* out_resets, float* out_extras, void* stream) {
  if (!h || !readback || !actions) return fail(LM_EINVAL, "lm_task_eval: null argument");
  CHECK_DEVICE(h, "lm_task_eval");
  hipStream_t s = (hipStream_t)stream;
  StepArgs A = make_args(h, actions, nullptr, out_obs, out_states, out_rew, out_resets); A.W.out_extras = out_extras;
  hipLaunchKernelGGL(k_task_eval, dim3(h->nblocks), dim3(64), 0, s, A, readback);
  HIPCHK(hipGetLastError());
  return LM_OK;
}

int lm_apply_resets(lm_engine* h, const float* goal_rand, void* stream) {
  if (!h) return fail(LM_EINVAL, "lm_apply_resets: null handle");
  CHECK_DEVICE(h, "lm_apply_resets");
  hipStream_t s = (hipStream_t)stream;
  StepArgs A = make_args(h, nullptr, goal_rand, nullptr, nullptr, nullptr, nullptr);
  hipLaunchKernelGGL(k_apply_resets, dim3(h->nblocks), dim3(64), 0, s, A);
  hipLaunchKernelGGL(k_apply_resets_cnt, dim3((h->N + 63) / 64), dim3(64), 0, s, h->d_cnt, h->N);
  HIPCHK(hipGetLastError());
  return LM_OK;
}

int lm_substeps(lm_engine* h, const float* targets, int n, void* stream) {
  if (!h || !targets || n < 0) return fail(LM_EINVAL, "lm_substeps: bad argument");
  CHECK_DEVICE(h, "lm_substeps");
  StepArgs A = make_args(h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  hipLaunchKernelGGL(h->contact_on ? k_substeps_cf : k_substeps, dim3(h->nblocks), dim3(64), 0, (hipStream_t)stream, A, targets, n);
  HIPCHK(hipGetLastError());
  return LM_OK;
}

int lm_forward_kinematics(lm_engine* h, float* tips, float* knees, void* stream) {
  if (!h || !tips || !knees) return fail(LM_EINVAL, "lm_forward_kinematics: null argument");
  CHECK_DEVICE(h, "lm_forward_kinematics");
  StepArgs A = make_args(h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  hipLaunchKernelGGL(k_fk, dim3(h->nblocks), dim3(64), 0, (hipStream_t)stream, A, tips, knees);
  HIPCHK(hipGetLastError());
  return LM_OK;
}

int lm_debug_dynamics(lm_engine* h, float* M, float* hvec, void* stream) {
  if (!h || !M || !hvec) return fail(LM_EINVAL, "lm_debug_dynamics: null argument");
  CHECK_DEVICE(h, "lm_debug_dynamics");
  if (h->h_params[0].mode != LM_MODE_LOCO || h->n_tasks != 1) return fail(LM_EINVAL, "lm_debug_dynamics: loco engines only");
  StepArgs A = make_args(h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  hipLaunchKernelGGL(k_debug_dyn, dim3(h->nblocks), dim3(64), 0, (hipStream_t)stream, A, M, hvec);
  HIPCHK(hipGetLastError());
  return LM_OK;
}

void* lm_ptr(lm_engine* h, int kind) {
  if (!h) return nullptr;
  switch (kind) {
    case LM_PTR_STATE: return h->d_state;
    case LM_PTR_CNT: return h->d_cnt;
    case LM_PTR_DR_CNT: return h->d_drc;
    case LM_PTR_DR_PHYS: return h->d_dr_phys;
    case LM_PTR_DR_RESET_STATE: return h->d_reset_dr ? (void*)(h->d_reset_dr + 2) : nullptr;
    case LM_PTR_DR_MASS: return h->d_mass_dr ? (void*)(h->d_mass_dr + 2) : nullptr;
    case LM_PTR_DR_ACTUATOR: return h->d_actuator_dr ? (void*)(h->d_actuator_dr + 2) : nullptr;
    case LM_PTR_OBS_BUF: h->view_obs = true; return h->d_obs;
    case LM_PTR_STATES_BUF: h->view_states = true; return h->d_states;
    case LM_PTR_REW_BUF: return h->d_rew;
    case LM_PTR_EXTRAS: return h->d_extras;
    case LM_PTR_STATS: return h->d_stats;
    case LM_PTR_TERMS: h->view_terms = true; return h->d_terms;
    case LM_PTR_CONTACT: return h->d_contact;
    case LM_PTR_ENV_PARAMS: return h->d_env_params;
    default: return nullptr;
  }
}
int lm_num_envs(const lm_engine* h) { return h ? h->N : 0; }
int lm_num_obs(const lm_engine* h) { return h ? h->num_obs : 0; }
int lm_set_seed(lm_engine* h, uint32_t seed) { if (!h) return fail(LM_EINVAL, "lm_set_seed: null handle"); h->seed = seed; return LM_OK; }

}  // extern "C"

// (lm_internal.h) the persistent rollout launch used by lm_rollout_run (lm_policy.hip)
int lm_internal_rollout(lm_engine* h, int policy, const LmRolloutArgs& R, hipStream_t s) {
  if (!h || !R.params || !R.log_std || !R.obs || !R.actions || !R.logp || !R.values || !R.rewards || !R.dones || !R.acc_steps || R.T <= 0) return -1;
  if (h->dr_enabled || R.nobs != h->num_obs) return fail(-1, "persistent rollout: domain-randomised engines and foreign observation widths run through the graph mode");
  if (h->contact_on) return fail(-1, "persistent rollout: an engine with contact-force reporting on runs through the graph mode");
  if (!on_device(h)) return fail(-1, "persistent rollout: the calling thread's current device is not the engine's device");
  StepArgs A = make_args(h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (!h->view_obs) A.W.obs_buf = nullptr;           // as the graph mode's lm_step(out_obs = the rollout's slot, out_states = NULL) does
  if (!h->view_terms) A.W.terms = nullptr;
  RolloutDev D; D.params = R.params; D.log_std = R.log_std; D.obs = R.obs; D.actions = R.actions; D.logp = R.logp; D.values = R.values;
  D.rewards = R.rewards; D.dones = R.dones; D.acc_steps = R.acc_steps; D.T = R.T; D.noise_seed = R.noise_seed;
  static const bool streaming = getenv("LM_ROLLOUT_STREAMING_MLP") != nullptr;      // kernel experiments: the four-wavefront tile with streamed weights
  const int ev = (R.deterministic ? LM_EV_DET : 0) | (R.record ? LM_EV_REC : 0);
  RolloutEv E; E.record = R.record; E.cap = R.episode_cap;
  if (R.traj_K) {      // builds that keep a trajectory record (lm_engine_tr.hip)
    if (!lm_internal_rollout_trajectories(policy, R.nobs, R.deterministic, R.record != nullptr)) return fail(-1, "persistent rollout: no build keeps a trajectory record for this policy / observation width / switches; such plans run through the graph mode");
    RolloutTraj TJ; TJ.ids = R.traj_ids; TJ.rows = R.traj_rows; TJ.header = R.traj_header; TJ.K = R.traj_K; TJ.max_rows = R.traj_max_rows; TJ.cap = R.traj_cap;
    if (lm_internal_launch_rollout_tr(&A, &D, &E, &TJ, ev | LM_EV_TRAJ, policy, R.nobs, h->nblocks, s)) return -1;
  }
  else if (ev) {      // evaluation builds (lm_engine_ev.hip; the MLP always on the resident tile)
    if (R.record && !lm_internal_rollout_records(policy, R.nobs)) return fail(-1, "persistent rollout: no recording build for this policy / observation width; recording plans run through the graph mode");
    if (lm_internal_launch_rollout_ev(&A, &D, &E, ev, policy, R.nobs, h->nblocks, s)) return -1;
  }
  else if (policy == LM_POLICY_MLP && R.nobs == 64 && !streaming) hipLaunchKernelGGL(k_rollout_mlp<64>, dim3(h->nblocks), dim3(256), 0, s, A, D);
  else if (policy == LM_POLICY_MLP && R.nobs == LM_MAX_OBS && !streaming) hipLaunchKernelGGL(k_rollout_mlp<LM_MAX_OBS>, dim3(h->nblocks), dim3(256), 0, s, A, D);
  else if (policy == LM_POLICY_MLP && R.nobs == 64) hipLaunchKernelGGL((k_rollout<64, LM_POLICY_MLP>), dim3(h->nblocks), dim3(256), 0, s, A, D);
  else if (policy == LM_POLICY_MLP && R.nobs == LM_MAX_OBS) hipLaunchKernelGGL((k_rollout<LM_MAX_OBS, LM_POLICY_MLP>), dim3(h->nblocks), dim3(256), 0, s, A, D);
  else if (policy == LM_POLICY_GNN && R.nobs == 64) hipLaunchKernelGGL((k_rollout<64, LM_POLICY_GNN>), dim3(h->nblocks), dim3(256), 0, s, A, D);
  else return -1;
  hipLaunchKernelGGL(k_rollout_finalize, dim3(1), dim3(64), 0, s, h->d_params, A.W, h->N, R.acc_steps, R.extras, R.T);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int lm_internal_rollout_supported(const lm_engine* h, int policy, int nobs) {
  if (!h || h->dr_enabled || h->contact_on || nobs != h->num_obs) return 0;
  return (policy == LM_POLICY_MLP && (nobs == 64 || nobs == LM_MAX_OBS)) || (policy == LM_POLICY_GNN && nobs == 64);
}

// Recording builds of the persistent kernels exist only where they compile without scratch memory: the resident MLP tile on 64-wide
// observations.  (With the record, the 88-wide MLP build needs 116 - 156 bytes of scratch per lane against 60 - 72 without and the GNN build
// 268 - 292 against 236 - 240: not shipped; those plans record in the graph mode.)
int lm_internal_rollout_records(int policy, int nobs) { return policy == LM_POLICY_MLP && nobs == 64; }
int lm_internal_rollout_trajectories(int policy, int nobs, int deterministic, int episode_record) {
  return lm_internal_rollout_tr_built(LM_EV_TRAJ | (deterministic ? LM_EV_DET : 0) | (episode_record ? LM_EV_REC : 0), policy, nobs);
}
int lm_internal_on_device(const lm_engine* h) { return h && on_device(h); }
void lm_internal_episode_info(const lm_engine* h, int* split, int* max_episode) {
  *split = h->split; max_episode[0] = h->h_params[0].max_episode; max_episode[1] = h->h_params[h->n_tasks == 2 ? 1 : 0].max_episode;
}
void lm_internal_trajectory_info(const lm_engine* h, int* split, int* free_body_row) {
  *split = h->split;
  for (int b = 0; b < 2; b++) free_body_row[b] = h->h_params[h->n_tasks == 2 ? b : 0].mode == LM_MODE_LOCO ? R_FB0 : R_FB1;
}
void lm_internal_replay_info(const lm_engine* h, int* variant, int* drive_mode, int* num_obs, int* split, float* act_scale, float* act_scale_se) {
  for (int b = 0; b < 2; b++) {
    const lm_params& p = h->h_params[h->n_tasks == 2 ? b : 0];
    variant[b] = p.variant; drive_mode[b] = p.drive_mode; num_obs[b] = p.num_obs;
    if (act_scale) act_scale[b] = p.act_scale;
    if (act_scale_se) act_scale_se[b] = p.act_scale_se;
  }
  if (split) *split = h->split;
}

uint64_t lm_internal_args_key(const lm_engine* h) {
  return h ? ((uint64_t)h->seed | ((uint64_t)((h->view_obs ? 1 : 0) | (h->view_states ? 2 : 0) | (h->view_terms ? 4 : 0) | (h->contact_on ? 8 : 0) | (h->d_env_params ? 16 : 0)) << 32)) : 0ull;
}
int lm_internal_fail(int code, const char* msg) { return fail(code, msg); }
