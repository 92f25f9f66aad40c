// lm_internal.h -- host-side hooks between lm_engine.hip and lm_policy.hip (one shared library; not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct lm_engine;

// buffers of a rollout plan (include/lm_policy.h lm_rollout_create), as the persistent rollout kernel needs them
struct LmRolloutArgs {
  const float* params; const float* log_std;
  float *obs, *actions, *logp, *values, *rewards, *extras; int64_t* dones;
  long long* acc_steps;        // [T][16] int64 accumulators, zero on entry; left zero
  int T, nobs; uint32_t noise_seed;
  int deterministic;           // lm_rollout_set_deterministic: the *_ev instantiations with the mean-action epilogue
  float* record; int episode_cap;      // lm_rollout_set_episode_record (record may be null: no recording)
  const int32_t* traj_ids; int traj_K; float* traj_rows; int32_t* traj_header; int traj_max_rows, traj_cap;      // lm_rollout_set_trajectory_record (traj_K 0: off)
};

// T x (policy forward -> sampling -> step) + the bootstrap forward in ONE kernel launch (lm_engine.hip); policy = LM_POLICY_MLP / _GNN.
// Returns 0, or a negative code when the engine cannot run it (domain-randomised engines; the GNN on 88-wide observations).
int lm_internal_rollout(lm_engine* h, int policy, const LmRolloutArgs& R, hipStream_t s);
// 1 when lm_internal_rollout can run this engine / policy / observation width
int lm_internal_rollout_supported(const lm_engine* h, int policy, int nobs);
// 1 when the persistent kernel has a build that keeps the episode record for this policy / observation width (else recording plans take the graph)
int lm_internal_rollout_records(int policy, int nobs);
// its twin for the trajectory record: 1 when the persistent kernel has a build that keeps one for this policy / observation width together with these
// other switches (deterministic actions, an episode record attached); else plans with a trajectory record take the graph
int lm_internal_rollout_trajectories(int policy, int nobs, int deterministic, int episode_record);
// 1 when the calling thread's current device is the engine's
int lm_internal_on_device(const lm_engine* h);
// what the episode record needs of the engine: first env of the second parameter block (N when there is one block) and max_episode of both
void lm_internal_episode_info(const lm_engine* h, int* split, int* max_episode);
// what the trajectory record needs of the engine: the same split, and per parameter block the state row its free body starts at (R_FB0, the
// base, for a locomotion block; R_FB1, the plate, for a manipulation block)
void lm_internal_trajectory_info(const lm_engine* h, int* split, int* free_body_row);
// what a replay plan (lm_replay.hip) checks of the engine: per parameter block (both entries the same with one block) the task variant, the
// drive mode and the observation width; for a PD plan also (each may be null) the first env of the second block (N with one block) and per
// block the action scales of the step: act_scale (variant 0) and act_scale_se (variants 1 / 2)
void lm_internal_replay_info(const lm_engine* h, int* variant, int* drive_mode, int* num_obs, int* split, float* act_scale, float* act_scale_se);
// what a captured lm_step launch has baked into its kernel arguments and the engine may change afterwards: the goal / domain-randomisation seed
// (lm_set_seed), which of the unclipped views are kept current (lm_ptr), and which kernels lm_step launches (lm_enable_contact_forces,
// lm_enable_env_params).  A hipGraph captured under another key is re-captured.
uint64_t lm_internal_args_key(const lm_engine* h);
// records a message for lm_last_error() (thread-local, lm_engine.hip) and returns `code`
int lm_internal_fail(int code, const char* msg);
