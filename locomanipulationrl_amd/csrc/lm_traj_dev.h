// lm_traj_dev.h -- the trajectory record of include/lm_policy.h on the device: the column map of a row and the update of one slot by one
// wavefront (lane = column), used by k_trajectory_update (lm_policy.hip); the column map also by the persistent builds that record
// (lm_engine_tr.hip; their device code and host hooks are in lm_rollout_dev.h), whose flag bit and argument block are declared here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/lm_policy.h"

// The state rows a trajectory row copies: the R_* rows of lm_dynamics.h, restated because the policy unit does not see the step's headers
// (checked where both are visible).
#define TRAJ_R_Q 13
#define TRAJ_R_QD 25
#define TRAJ_R_LACT 50
#define TRAJ_R_LTIP 74
#define TRAJ_R_GOAL 86
#ifdef R_Q
static_assert(TRAJ_R_Q == R_Q && TRAJ_R_QD == R_QD && TRAJ_R_LACT == R_LACT && TRAJ_R_LTIP == R_LTIP && TRAJ_R_GOAL == R_GOAL, "trajectory rows follow lm_dynamics.h");
#endif
static_assert(LM_TRAJ_COLS == 64, "one lane of a wavefront per column");

// Persistent builds with the record (lm_engine_tr.hip): a third bit of the EV flag of lm_rollout_dev.h, and the arguments that travel next to
// RolloutEv (StepArgs, SampleArgs and RolloutDev keep their size).
#define LM_EV_TRAJ 4
struct RolloutTraj { const int32_t* ids; float* rows; int32_t* header; int K, max_rows, cap; };

// column c of a row -> the state row it copies (fb: R_FB0 or R_FB1 of the env's block), or -1 for columns 59..63 (step outputs and counters)
__device__ __forceinline__ int traj_state_row(int c, int fb) {
  return c < 12 ? TRAJ_R_Q + c : c < 24 ? TRAJ_R_QD + (c - 12) : c < 31 ? fb + (c - 24) : c < 43 ? TRAJ_R_LACT + (c - 31) :
         c < 55 ? TRAJ_R_LTIP + (c - 43) : c < 59 ? TRAJ_R_GOAL + (c - 55) : -1;
}

// the word of column c for env (0 <= env < N) after a step: a copy, nothing else
__device__ __forceinline__ float traj_word(const float* __restrict__ state, const int64_t* __restrict__ cnt, const float* __restrict__ rewards,
                                           const int64_t* __restrict__ dones, size_t N, size_t env, int fb, int c) {
  const int sr = traj_state_row(c, fb);
  if (sr >= 0) return state[(size_t)sr * N + env];
  if (c == 59) return rewards[env];
  if (c == 60) return dones[env] != 0 ? 1.0f : 0.0f;
  if (c == 61) return cnt[2 * N + env] != 0 ? 1.0f : 0.0f;                 // goal_reset_buf
  return (float)cnt[(c == 62 ? 4 : 5) * N + env];                          // progress_buf | episode_count
}

// One slot, one wavefront: every lane reads the slot's header (a uniform value), lane c stores column c of the new row - the row is one contiguous
// 256-byte segment - and lane 0 writes the header back.  The header's new words depend on the loaded ones, so no store overtakes the loads.
__device__ __forceinline__ void traj_update_slot(const float* __restrict__ state, const int64_t* __restrict__ cnt, const float* __restrict__ rewards,
                                                 const int64_t* __restrict__ dones, int N, int env, int fb, float* __restrict__ slot_rows,
                                                 int32_t* __restrict__ hdr, int max_rows, int cap, int lane) {
  const int nrows = hdr[0], episodes = hdr[1];
  if (cap > 0 && episodes >= cap) return;
  const bool done = dones[env] != 0;
  const bool room = nrows >= 0 && nrows < max_rows;            // (a header the caller filled with garbage cannot send a store outside the slot)
  if (room) slot_rows[(size_t)nrows * LM_TRAJ_COLS + lane] = traj_word(state, cnt, rewards, dones, (size_t)N, (size_t)env, fb, lane);
  if (lane == 0) {
    if (room) hdr[0] = nrows + 1; else hdr[2] += 1;
    if (done) hdr[1] = episodes + 1;
  }
}
