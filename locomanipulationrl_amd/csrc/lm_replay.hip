// lm_replay.hip -- replay of recorded joint motions (include/lm_policy.h, "replay of recorded joint motions"): the plan (device copies of the
// recordings, their action tables and the env -> recording map) and the one small kernel a caller launches between lm_step calls, which
// scores every env against its recording and writes the actions of the next step.  No step kernel is touched: the kernel reads what lm_step
// left in the engine's state and counters and in the step's outputs, as k_episode_update and k_trajectory_update do.
// Two kinds of plan: the velocity-drive one (lm_replay_create, k_replay_update) and the PD-actuator one (lm_replay_create_pd,
// k_replay_update_pd), whose table holds logged actions or logged joint position targets.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/lm_policy.h"
#include "../../include/lm_engine.h"
#include "lm_internal.h"
#include <new>

// The state rows the kernel reads: R_Q of lm_dynamics.h, restated because this unit does not see the step's headers (lm_traj_dev.h does the same).
#define REPLAY_R_Q 13
#ifdef R_Q
static_assert(REPLAY_R_Q == R_Q, "replay rows follow lm_dynamics.h");
#endif
#define REPLAY_R_SE 90      // the swing / extension position targets of variants 1 / 2 (the PD kernel only)
#ifdef R_SE
static_assert(REPLAY_R_SE == R_SE, "replay rows follow lm_dynamics.h");
#endif
static_assert(LM_NUM_OBS == 64 && LM_NUM_ACTIONS == 12, "the replay kernel reads 64-wide observations and writes 12 actions");

// rows of the record (include/lm_policy.h)
enum { RP_ROWS = 0, RP_FINISHED = 1, RP_DONE_AT = 2, RP_GOAL = 3, RP_ROW0_ERR = 4, RP_QERR = 5, RP_SQ_SUM = 6, RP_TRACKED = 7, RP_EARLY = 8, RP_FIRST_SUCC = 9,
       RP_IN_WINDOW = 10, RP_MIN_V2 = 11, RP_RET = 12, RP_WINDOW_RETURN = 13, RP_V2_FIRST = 14, RP_ABS_SUM = 15, RP_QPREV = 16, RP_SATURATED = 28, RP_CMD_ERR = 29 };
static_assert(RP_QPREV + 12 <= RP_SATURATED && RP_CMD_ERR < LM_REPLAY_ROWS, "the record holds qprev and the two rows of a PD plan");

struct lm_replay {
  lm_engine* env;
  float* d_rec; float* d_act; int32_t* d_len; int32_t* d_env_rec;
  int N, R, T_max, servo, hold, window_rows, steps;
  float inv_full, v2_thresh, track_tol;
  // a PD plan (kind 1; d_act holds the command table): command mode, observation width, first env of the second block, and per block the task
  // variant and the reciprocal of the scale its step applies to an action (act_scale_se for variants 1 / 2, act_scale for variant 0)
  int kind, cmd_mode, nobs, split, variant[2];
  float inv_scale[2];
};

struct ReplayArgs {
  const float* state; const int64_t* cnt; const float* obs; const float* rewards;
  const float* rec; const float* act; const int32_t* len; const int32_t* env_rec;
  float* record; float* actions_next;
  int N, R, T_max, s, servo, hold, window_rows;
  float inv_full, v2_thresh, track_tol;
};

__device__ __forceinline__ void replay_store_actions(float* __restrict__ dst, const float* a) {      // one env's 12 actions: three 16-byte stores (48 e is a multiple of 16)
  float4* d4 = reinterpret_cast<float4*>(dst);
  d4[0] = make_float4(a[0], a[1], a[2], a[3]); d4[1] = make_float4(a[4], a[5], a[6], a[7]); d4[2] = make_float4(a[8], a[9], a[10], a[11]);
}

// One thread per env.  Every access to state, counters and record is row-major over the envs (lane = env: coalesced); the recording rows are read
// through the env's own recording id (envs of a block that replay the same recording read the same 48 bytes).
__global__ void __launch_bounds__(256) k_replay_update(ReplayArgs A) {
#pragma clang fp contract(off)
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= A.N) return;
  const size_t N = (size_t)A.N, e = (size_t)env;
  const int s = A.s;
  float an[12];
#pragma unroll
  for (int j = 0; j < 12; j++) an[j] = 0.f;
  float* __restrict__ out = A.actions_next + e * 12;
  const int r = A.env_rec[env];
  if (r < 0 || r >= A.R) { replay_store_actions(out, an); return; }      // the env takes no part: zero actions, its record column is not touched
  float* __restrict__ rc = A.record + e;
  const int T = A.len[r];
  bool finished = rc[RP_FINISHED * N] != 0.f;
  if (finished || s >= T + A.hold) { replay_store_actions(out, an); return; }
  float q[12];
#pragma unroll
  for (int j = 0; j < 12; j++) q[j] = A.state[(size_t)(REPLAY_R_Q + j) * N + e];
  const float* __restrict__ o = A.obs + e * LM_NUM_OBS;
  const float o7 = o[7], o8 = o[8], o9 = o[9];
  const float v2 = (o7 * o7 + o8 * o8) + o9 * o9;
  const float rew = A.rewards[env];
  const float* __restrict__ recr = A.rec + (size_t)r * (size_t)A.T_max * 12;
  if (s < T) {      // s < T <= T_max: row s of the recording exists
    const float* __restrict__ row = recr + (size_t)s * 12;
    float rs[12], d[12], m = 0.f, sa = 0.f, sq = 0.f;
#pragma unroll
    for (int j = 0; j < 12; j++) { rs[j] = row[j]; d[j] = q[j] - rs[j]; m = fmaxf(m, fabsf(d[j])); sa += fabsf(d[j]); sq += d[j] * d[j]; }
    if (s == 0) { rc[RP_ROW0_ERR * N] = m; rc[RP_V2_FIRST * N] = v2; }
    rc[RP_QERR * N] = fmaxf(rc[RP_QERR * N], m);
    rc[RP_ABS_SUM * N] += sa;
    rc[RP_SQ_SUM * N] += sq;
    if (s >= 1) {
      const float* __restrict__ prow = row - 12;
      float se = 0.f; int tracked = 0;
#pragma unroll
      for (int j = 0; j < 12; j++) {
        const float ej = (q[j] - rc[(size_t)(RP_QPREV + j) * N]) - (rs[j] - prow[j]);
        tracked += fabsf(ej) < A.track_tol ? 1 : 0; se += fabsf(ej);
      }
      rc[RP_TRACKED * N] += (float)tracked;
      if (s <= 4) rc[RP_EARLY * N] += se;
    }
    const bool win = s >= T - A.window_rows;
    if (v2 <= A.v2_thresh) {
      if (rc[RP_FIRST_SUCC * N] < 0.f) rc[RP_FIRST_SUCC * N] = (float)s;
      if (win) rc[RP_IN_WINDOW * N] += 1.f;
    }
    rc[RP_MIN_V2 * N] = fminf(rc[RP_MIN_V2 * N], v2);
    if (win) rc[RP_WINDOW_RETURN * N] += rew;
    rc[RP_ROWS * N] += 1.f;
#pragma unroll
    for (int j = 0; j < 12; j++) rc[(size_t)(RP_QPREV + j) * N] = q[j];
  }
  rc[RP_RET * N] += rew;
  if (A.cnt[3 * N + e] != 0) {
    finished = true;
    rc[RP_FINISHED * N] = 1.f; rc[RP_DONE_AT * N] = (float)s; rc[RP_GOAL * N] = A.cnt[2 * N + e] != 0 ? 1.f : 0.f;
  }
  if (!finished && s + 1 < T) {      // s + 1 < T <= T_max: row s + 1 of both tables exists
    if (A.servo) {
      const float* __restrict__ nrow = recr + (size_t)(s + 1) * 12;
#pragma unroll
      for (int j = 0; j < 12; j++) an[j] = fminf(fmaxf((nrow[j] - q[j]) * A.inv_full, -1.f), 1.f);
    } else {
      const float* __restrict__ arow = A.act + ((size_t)r * (size_t)A.T_max + (size_t)(s + 1)) * 12;
#pragma unroll
      for (int j = 0; j < 12; j++) an[j] = arow[j];
    }
  }
  replay_store_actions(out, an);
}

struct ReplayPdArgs {
  const float* state; const int64_t* cnt; const float* obs; const float* rewards;
  const float* rec; const float* cmd; const int32_t* len; const int32_t* env_rec;
  float* record; float* actions_next;
  int N, R, T_max, s, targets, hold, window_rows, nobs, split, variant0, variant1;
  float inv_scale0, inv_scale1, v2_thresh, track_tol;
};

// joint position targets (joint order of rec) -> the swing / extension command of variants 1 / 2: the inverse of tgtq in lm_step.h
__device__ __forceinline__ void replay_se_command(const float* __restrict__ t, float* c) {
#pragma clang fp contract(off)
#pragma unroll
  for (int l = 0; l < 4; l++) { c[l] = t[l]; c[4 + 2 * l] = 0.5f * (t[4 + 2 * l] + t[5 + 2 * l]); c[5 + 2 * l] = t[4 + 2 * l] - t[5 + 2 * l]; }
}

// The PD twin of k_replay_update: the same scoring (rows 0..27, finished, hold, the window) on obs rows of the engine's width, the next action
// from the command table - a copy (actions mode) or the action that moves the engine's held command onto the logged targets (targets mode) -
// and rows 28 (saturated) and 29 (cmd_err).  One thread per env, SoA accesses, no atomics, no LDS.
__global__ void __launch_bounds__(256) k_replay_update_pd(ReplayPdArgs A) {
#pragma clang fp contract(off)
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= A.N) return;
  const size_t N = (size_t)A.N, e = (size_t)env;
  const int s = A.s;
  float an[12];
#pragma unroll
  for (int j = 0; j < 12; j++) an[j] = 0.f;
  float* __restrict__ out = A.actions_next + e * 12;
  const int r = A.env_rec[env];
  if (r < 0 || r >= A.R) { replay_store_actions(out, an); return; }
  float* __restrict__ rc = A.record + e;
  const int T = A.len[r];
  bool finished = rc[RP_FINISHED * N] != 0.f;
  if (finished || s >= T + A.hold) { replay_store_actions(out, an); return; }
  const bool second = env >= A.split;
  const int variant = second ? A.variant1 : A.variant0;
  const float inv_scale = second ? A.inv_scale1 : A.inv_scale0;
  const bool se_cmd = A.targets && variant >= 1;      // the command lives in the swing / extension rows
  float q[12], se[12];
#pragma unroll
  for (int j = 0; j < 12; j++) q[j] = A.state[(size_t)(REPLAY_R_Q + j) * N + e];
#pragma unroll
  for (int j = 0; j < 12; j++) se[j] = se_cmd ? A.state[(size_t)(REPLAY_R_SE + j) * N + e] : 0.f;
  const float* __restrict__ o = A.obs + e * (size_t)A.nobs;
  const float o7 = o[7], o8 = o[8], o9 = o[9];
  const float v2 = (o7 * o7 + o8 * o8) + o9 * o9;
  const float rew = A.rewards[env];
  const float* __restrict__ recr = A.rec + (size_t)r * (size_t)A.T_max * 12;
  const float* __restrict__ cmdr = A.cmd + (size_t)r * (size_t)A.T_max * 12;
  if (s < T) {      // s < T <= T_max: row s of both tables exists
    const float* __restrict__ row = recr + (size_t)s * 12;
    float rs[12], d[12], m = 0.f, sa = 0.f, sq = 0.f;
#pragma unroll
    for (int j = 0; j < 12; j++) { rs[j] = row[j]; d[j] = q[j] - rs[j]; m = fmaxf(m, fabsf(d[j])); sa += fabsf(d[j]); sq += d[j] * d[j]; }
    if (s == 0) { rc[RP_ROW0_ERR * N] = m; rc[RP_V2_FIRST * N] = v2; }
    rc[RP_QERR * N] = fmaxf(rc[RP_QERR * N], m);
    rc[RP_ABS_SUM * N] += sa;
    rc[RP_SQ_SUM * N] += sq;
    if (s >= 1) {
      const float* __restrict__ prow = row - 12;
      float se_ = 0.f; int tracked = 0;
#pragma unroll
      for (int j = 0; j < 12; j++) {
        const float ej = (q[j] - rc[(size_t)(RP_QPREV + j) * N]) - (rs[j] - prow[j]);
        tracked += fabsf(ej) < A.track_tol ? 1 : 0; se_ += fabsf(ej);
      }
      rc[RP_TRACKED * N] += (float)tracked;
      if (s <= 4) rc[RP_EARLY * N] += se_;
      if (se_cmd) {      // the command the engine holds after step s against the command logged for it
        float t[12], c[12], ce = 0.f;
        const float* __restrict__ crow = cmdr + (size_t)s * 12;
#pragma unroll
        for (int j = 0; j < 12; j++) t[j] = crow[j];
        replay_se_command(t, c);
#pragma unroll
        for (int j = 0; j < 12; j++) ce = fmaxf(ce, fabsf(c[j] - se[j]));
        rc[RP_CMD_ERR * N] = fmaxf(rc[RP_CMD_ERR * N], ce);
      }
    }
    const bool win = s >= T - A.window_rows;
    if (v2 <= A.v2_thresh) {
      if (rc[RP_FIRST_SUCC * N] < 0.f) rc[RP_FIRST_SUCC * N] = (float)s;
      if (win) rc[RP_IN_WINDOW * N] += 1.f;
    }
    rc[RP_MIN_V2 * N] = fminf(rc[RP_MIN_V2 * N], v2);
    if (win) rc[RP_WINDOW_RETURN * N] += rew;
    rc[RP_ROWS * N] += 1.f;
#pragma unroll
    for (int j = 0; j < 12; j++) rc[(size_t)(RP_QPREV + j) * N] = q[j];
  }
  rc[RP_RET * N] += rew;
  if (A.cnt[3 * N + e] != 0) {
    finished = true;
    rc[RP_FINISHED * N] = 1.f; rc[RP_DONE_AT * N] = (float)s; rc[RP_GOAL * N] = A.cnt[2 * N + e] != 0 ? 1.f : 0.f;
  }
  if (!finished && s + 1 < T) {      // s + 1 < T <= T_max: row s + 1 of the command table exists
    const float* __restrict__ nrow = cmdr + (size_t)(s + 1) * 12;
    float t[12];
#pragma unroll
    for (int j = 0; j < 12; j++) t[j] = nrow[j];
    if (A.targets) {
      float c[12]; int sat = 0;
      if (variant >= 1) replay_se_command(t, c);
      else {
#pragma unroll
        for (int j = 0; j < 12; j++) c[j] = t[j];
      }
#pragma unroll
      for (int j = 0; j < 12; j++) {
        const float raw = (c[j] - se[j]) * inv_scale;      // se = 0 for variant 0 in position drive: c - 0 is c exactly
        sat += fabsf(raw) > 1.f ? 1 : 0;
        an[j] = fminf(fmaxf(raw, -1.f), 1.f);
      }
      rc[RP_SATURATED * N] += (float)sat;
    } else {
#pragma unroll
      for (int j = 0; j < 12; j++) an[j] = t[j];
    }
  }
  replay_store_actions(out, an);
}

static bool all_finite(const float* a, size_t n) { for (size_t i = 0; i < n; i++) if (!isfinite(a[i])) return false; return true; }

extern "C" {

int lm_replay_create(lm_replay** out, lm_engine* h, const float* rec_host, const float* act_host, const int32_t* len_host, int R, int T_max,
                     const int32_t* env_rec_host, int servo, int hold, int window_rows, float inv_full, float v2_thresh, float track_tol) {
  if (!out || !h || !rec_host || !act_host || !len_host || !env_rec_host) return lm_internal_fail(LM_EINVAL, "lm_replay_create: null out, engine, rec, act, len or env_rec");
  *out = nullptr;
  if (R < 1 || T_max < 1) return lm_internal_fail(LM_EINVAL, "lm_replay_create: R and T_max must be at least 1");
  if (hold < 0 || hold > 8) return lm_internal_fail(LM_EINVAL, "lm_replay_create: hold must be in [0, 8]");
  if (window_rows < 1) return lm_internal_fail(LM_EINVAL, "lm_replay_create: window_rows must be at least 1");
  if (!isfinite(inv_full) || !isfinite(v2_thresh) || !isfinite(track_tol)) return lm_internal_fail(LM_EINVAL, "lm_replay_create: inv_full, v2_thresh and track_tol must be finite");
  for (int r = 0; r < R; r++)
    if (len_host[r] < window_rows || len_host[r] > T_max) return lm_internal_fail(LM_EINVAL, "lm_replay_create: a recording's length is outside [window_rows, T_max]");
  const size_t words = (size_t)R * (size_t)T_max * 12;
  if (!all_finite(rec_host, words) || !all_finite(act_host, words)) return lm_internal_fail(LM_EINVAL, "lm_replay_create: a table entry is not finite");
  if (!lm_internal_on_device(h)) return lm_internal_fail(LM_EINVAL, "lm_replay_create: the calling thread's current device is not the engine's device");
  int variant[2], drive[2], nobs[2]; lm_internal_replay_info(h, variant, drive, nobs, nullptr, nullptr, nullptr);
  for (int b = 0; b < 2; b++)
    if (variant[b] != 0 || drive[b] != LM_DRIVE_VELOCITY || nobs[b] != LM_NUM_OBS)
      return lm_internal_fail(LM_EINVAL, "lm_replay_create: every block must be variant 0 in velocity drive with 64-wide observations (PD targets are not joint-rate actions)");
  const int N = lm_num_envs(h);
  int steps = 0;
  for (int e = 0; e < N; e++) {
    const int32_t r = env_rec_host[e];
    if (r < -1 || r >= R) return lm_internal_fail(LM_EINVAL, "lm_replay_create: a recording id outside [-1, R)");
    if (r >= 0 && len_host[r] + hold > steps) steps = len_host[r] + hold;
  }
  lm_replay* p = new (std::nothrow) lm_replay();
  if (!p) return lm_internal_fail(LM_EHIP, "lm_replay_create: out of host memory");
  p->env = h; p->N = N; p->R = R; p->T_max = T_max; p->servo = servo ? 1 : 0; p->hold = hold; p->window_rows = window_rows; p->steps = steps;
  p->inv_full = inv_full; p->v2_thresh = v2_thresh; p->track_tol = track_tol;
  const bool ok = hipMalloc((void**)&p->d_rec, words * sizeof(float)) == hipSuccess && hipMalloc((void**)&p->d_act, words * sizeof(float)) == hipSuccess &&
                  hipMalloc((void**)&p->d_len, (size_t)R * sizeof(int32_t)) == hipSuccess && hipMalloc((void**)&p->d_env_rec, (size_t)N * sizeof(int32_t)) == hipSuccess &&
                  hipMemcpy(p->d_rec, rec_host, words * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(p->d_act, act_host, words * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(p->d_len, len_host, (size_t)R * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(p->d_env_rec, env_rec_host, (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) { lm_replay_destroy(p); return lm_internal_fail(LM_EHIP, "lm_replay_create: hipMalloc or hipMemcpy failed"); }
  *out = p;
  return LM_OK;
}

int lm_replay_create_pd(lm_replay** out, lm_engine* h, const float* rec_host, const float* cmd_host, const int32_t* len_host, int R, int T_max,
                        const int32_t* env_rec_host, int cmd_mode, int hold, int window_rows, float v2_thresh, float track_tol) {
  if (!out || !h || !rec_host || !cmd_host || !len_host || !env_rec_host) return lm_internal_fail(LM_EINVAL, "lm_replay_create_pd: null out, engine, rec, cmd, len or env_rec");
  *out = nullptr;
  if (R < 1 || T_max < 1) return lm_internal_fail(LM_EINVAL, "lm_replay_create_pd: R and T_max must be at least 1");
  if (cmd_mode != LM_REPLAY_CMD_ACTIONS && cmd_mode != LM_REPLAY_CMD_TARGETS) return lm_internal_fail(LM_EINVAL, "lm_replay_create_pd: cmd_mode must be LM_REPLAY_CMD_ACTIONS or LM_REPLAY_CMD_TARGETS");
  if (hold < 0 || hold > 8) return lm_internal_fail(LM_EINVAL, "lm_replay_create_pd: hold must be in [0, 8]");
  if (window_rows < 1) return lm_internal_fail(LM_EINVAL, "lm_replay_create_pd: window_rows must be at least 1");
  if (!isfinite(v2_thresh) || !isfinite(track_tol)) return lm_internal_fail(LM_EINVAL, "lm_replay_create_pd: v2_thresh and track_tol must be finite");
  for (int r = 0; r < R; r++)
    if (len_host[r] < window_rows || len_host[r] > T_max) return lm_internal_fail(LM_EINVAL, "lm_replay_create_pd: a recording's length is outside [window_rows, T_max]");
  const size_t words = (size_t)R * (size_t)T_max * 12;
  if (!all_finite(rec_host, words) || !all_finite(cmd_host, words)) return lm_internal_fail(LM_EINVAL, "lm_replay_create_pd: a table entry is not finite");
  if (!lm_internal_on_device(h)) return lm_internal_fail(LM_EINVAL, "lm_replay_create_pd: the calling thread's current device is not the engine's device");
  int variant[2], drive[2], nobs[2], split = 0; float act_scale[2], act_scale_se[2], inv_scale[2];
  lm_internal_replay_info(h, variant, drive, nobs, &split, act_scale, act_scale_se);
  for (int b = 0; b < 2; b++) {
    if (variant[b] == 0 && drive[b] != LM_DRIVE_POSITION)
      return lm_internal_fail(LM_EINVAL, drive[b] == LM_DRIVE_VELOCITY ? "lm_replay_create_pd: a block in velocity drive (lm_replay_create replays those)"
                                                                       : "lm_replay_create_pd: a block in effort drive (a torque is neither a target nor a PD command)");
    if (variant[b] < 0 || variant[b] > 2 || nobs[b] != lm_num_obs(h)) return lm_internal_fail(LM_EINVAL, "lm_replay_create_pd: a block of an unknown variant or observation width");
    inv_scale[b] = 1.0f / (variant[b] >= 1 ? act_scale_se[b] : act_scale[b]);      // formed once, in float
    if (!isfinite(inv_scale[b])) return lm_internal_fail(LM_EINVAL, "lm_replay_create_pd: a block whose action scale has no finite reciprocal");
  }
  const int N = lm_num_envs(h);
  int steps = 0;
  for (int e = 0; e < N; e++) {
    const int32_t r = env_rec_host[e];
    if (r < -1 || r >= R) return lm_internal_fail(LM_EINVAL, "lm_replay_create_pd: a recording id outside [-1, R)");
    if (r >= 0 && len_host[r] + hold > steps) steps = len_host[r] + hold;
  }
  lm_replay* p = new (std::nothrow) lm_replay();
  if (!p) return lm_internal_fail(LM_EHIP, "lm_replay_create_pd: out of host memory");
  p->env = h; p->N = N; p->R = R; p->T_max = T_max; p->hold = hold; p->window_rows = window_rows; p->steps = steps;
  p->v2_thresh = v2_thresh; p->track_tol = track_tol;
  p->kind = 1; p->cmd_mode = cmd_mode; p->nobs = lm_num_obs(h); p->split = split;
  for (int b = 0; b < 2; b++) { p->variant[b] = variant[b]; p->inv_scale[b] = inv_scale[b]; }
  const bool ok = hipMalloc((void**)&p->d_rec, words * sizeof(float)) == hipSuccess && hipMalloc((void**)&p->d_act, words * sizeof(float)) == hipSuccess &&
                  hipMalloc((void**)&p->d_len, (size_t)R * sizeof(int32_t)) == hipSuccess && hipMalloc((void**)&p->d_env_rec, (size_t)N * sizeof(int32_t)) == hipSuccess &&
                  hipMemcpy(p->d_rec, rec_host, words * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(p->d_act, cmd_host, words * sizeof(float), hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(p->d_len, len_host, (size_t)R * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(p->d_env_rec, env_rec_host, (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) { lm_replay_destroy(p); return lm_internal_fail(LM_EHIP, "lm_replay_create_pd: hipMalloc or hipMemcpy failed"); }
  *out = p;
  return LM_OK;
}

int lm_replay_steps(const lm_replay* p) { return p ? p->steps : lm_internal_fail(LM_EINVAL, "lm_replay_steps: null plan"); }

int lm_replay_update(lm_replay* p, int s, const float* obs, const float* rewards, float* record, float* actions_next, void* stream) {
  if (!p || !obs || !rewards || !record || !actions_next) return lm_internal_fail(LM_EINVAL, "lm_replay_update: null plan, obs, rewards, record or actions_next");
  if (s < 0) return lm_internal_fail(LM_EINVAL, "lm_replay_update: s must not be negative");
  if (reinterpret_cast<uintptr_t>(actions_next) & 15) return lm_internal_fail(LM_EINVAL, "lm_replay_update: actions_next must be 16-byte aligned");
  if (!lm_internal_on_device(p->env)) return lm_internal_fail(LM_EINVAL, "lm_replay_update: the calling thread's current device is not the engine's device");
  if (p->kind == 1) {
    ReplayPdArgs B;
    B.state = (const float*)lm_ptr(p->env, LM_PTR_STATE); B.cnt = (const int64_t*)lm_ptr(p->env, LM_PTR_CNT); B.obs = obs; B.rewards = rewards;
    B.rec = p->d_rec; B.cmd = p->d_act; B.len = p->d_len; B.env_rec = p->d_env_rec; B.record = record; B.actions_next = actions_next;
    B.N = p->N; B.R = p->R; B.T_max = p->T_max; B.s = s; B.targets = p->cmd_mode == LM_REPLAY_CMD_TARGETS ? 1 : 0; B.hold = p->hold; B.window_rows = p->window_rows;
    B.nobs = p->nobs; B.split = p->split; B.variant0 = p->variant[0]; B.variant1 = p->variant[1];
    B.inv_scale0 = p->inv_scale[0]; B.inv_scale1 = p->inv_scale[1]; B.v2_thresh = p->v2_thresh; B.track_tol = p->track_tol;
    hipLaunchKernelGGL(k_replay_update_pd, dim3((p->N + 255) / 256), dim3(256), 0, (hipStream_t)stream, B);
    return hipGetLastError() == hipSuccess ? LM_OK : LM_EHIP;
  }
  ReplayArgs A;
  A.state = (const float*)lm_ptr(p->env, LM_PTR_STATE); A.cnt = (const int64_t*)lm_ptr(p->env, LM_PTR_CNT); A.obs = obs; A.rewards = rewards;
  A.rec = p->d_rec; A.act = p->d_act; A.len = p->d_len; A.env_rec = p->d_env_rec; A.record = record; A.actions_next = actions_next;
  A.N = p->N; A.R = p->R; A.T_max = p->T_max; A.s = s; A.servo = p->servo; A.hold = p->hold; A.window_rows = p->window_rows;
  A.inv_full = p->inv_full; A.v2_thresh = p->v2_thresh; A.track_tol = p->track_tol;
  hipLaunchKernelGGL(k_replay_update, dim3((p->N + 255) / 256), dim3(256), 0, (hipStream_t)stream, A);
  return hipGetLastError() == hipSuccess ? LM_OK : LM_EHIP;
}

int lm_replay_destroy(lm_replay* p) {
  if (!p) return LM_OK;
  if (p->d_rec) hipFree(p->d_rec);
  if (p->d_act) hipFree(p->d_act);
  if (p->d_len) hipFree(p->d_len);
  if (p->d_env_rec) hipFree(p->d_env_rec);
  delete p;
  return LM_OK;
}

}  // extern "C"
