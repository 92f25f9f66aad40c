// lm_task.h -- device code of the step, layer 3 of 4: the task layer (observations, reward, termination) and the shared output tail with the
// fused reductions over envs.
#pragma once
#include "lm_dynamics.h"

// ------------------------------------------------------------------------------------------------
// task layer (obs / reward / termination), one env = 4 lanes; restates
// quadruped_pose_control.py:301-426,428-560,562-633 and quadruped_manipulate_plate.py:311-435,569-652
// ------------------------------------------------------------------------------------------------
struct TaskIn {
  float q[3], qd[3], acc[3], act[3];       // this limb's joints (dof1, dof2, dof3)
  float torque[3], tgtq[3];                // custom-controller tasks: logged torque, current joint position targets
  V3 tipw, knee2, knee3;                   // world positions of this limb's tip and knees
  V3 fp; Q4 fq; V3 lin, ang;               // free body (base or plate) world pose / velocity
};
struct TaskState { float lact[3]; V3 ltip; Q4 goal; int succ, consec, greset, reset, progress; float ltgt[3]; float lrd; };
struct TaskOut { float rew; float terms[11]; };

template <int MODE, int VAR>
LM_DEV void task_eval(const lm_params* __restrict__ P, int limb, int envl, const TaskIn& I, TaskState& S, TaskOut& O,
                      float* sObs, float* sSt) {
  S.progress += 1;
  // Every parameter the task layer reads, fetched in ONE batch of loads: read where they are used (inside || chains and after branches) each
  // one was a load the compiler may not hoist, i.e. an exposed cache round trip for the lone wavefront - twenty of them in a row.
  struct { float s_pos, s_lin, s_ang, s_q, s_qd, quat_scale, rot_eps, trans_scale, acc_scale, rate_scale, bonus, limit_pen, fall_pen, succ_thresh, h_base, h_corner, h_knee;
           float d23_pen[2], d23_rst[2], d1_pen[2], d1_rst[2], corner[3]; int max_consec, max_episode; } C;
  C.s_pos = P->s_pos; C.s_lin = P->s_lin; C.s_ang = P->s_ang; C.s_q = P->s_q; C.s_qd = P->s_qd; C.quat_scale = P->quat_scale; C.rot_eps = P->rot_eps;
  C.trans_scale = P->trans_scale; C.acc_scale = P->acc_scale; C.rate_scale = P->rate_scale; C.bonus = P->bonus; C.limit_pen = P->limit_pen;
  C.fall_pen = P->fall_pen; C.succ_thresh = P->succ_thresh; C.h_base = P->h_base; C.h_corner = P->h_corner; C.h_knee = P->h_knee;
  C.d23_pen[0] = P->d23_pen[0]; C.d23_pen[1] = P->d23_pen[1]; C.d23_rst[0] = P->d23_rst[0]; C.d23_rst[1] = P->d23_rst[1];
  C.d1_pen[0] = P->d1_pen[limb][0]; C.d1_pen[1] = P->d1_pen[limb][1]; C.d1_rst[0] = P->d1_rst[limb][0]; C.d1_rst[1] = P->d1_rst[limb][1];
  C.corner[0] = P->corner[limb][0]; C.corner[1] = P->corner[limb][1]; C.corner[2] = P->corner[limb][2];
  C.max_consec = P->max_consec; C.max_episode = P->max_episode;
  V3 opos, olin, oang; Q4 oq; M3 Rr; V3 pr;
  if (MODE == 0) {
    Rr = quat_to_mat(I.fq.w, I.fq.x, I.fq.y, I.fq.z); pr = I.fp;
    opos = mulT(Rr, -I.fp); oq = qconj(I.fq); olin = mulT(Rr, -I.lin); oang = mulT(Rr, -I.ang);
  } else {
    Q4 qr; qr.w = P->fixed_base_quat[0]; qr.x = P->fixed_base_quat[1]; qr.y = P->fixed_base_quat[2]; qr.z = P->fixed_base_quat[3];
    Rr = quat_to_mat(qr.w, qr.x, qr.y, qr.z); pr = v3(P->fixed_base_pos[0], P->fixed_base_pos[1], P->fixed_base_pos[2]);
    opos = mulT(Rr, I.fp - pr);
    oq = qmul(qconj(qr), I.fq);
    if (oq.w < 0.f) { oq.w = -oq.w; oq.x = -oq.x; oq.y = -oq.y; oq.z = -oq.z; }
    olin = mulT(Rr, I.lin); oang = mulT(Rr, I.ang);
  }
  V3 btip = mulT(Rr, I.tipw - pr);
  Q4 qd_ = qmul(oq, qconj(S.goal));
  constexpr bool var1 = (VAR == 1), var2 = (VAR == 2), pd = (VAR >= 1); const int NO = var1 ? LM_MAX_OBS : 64;
  float fl = (qd_.w < 0.f && !var1) ? -1.f : 1.f;        // the custom-controller tasks do not flip the sign (…custom_controller.py:429-431)
  Q4 qf; qf.w = fl * qd_.w; qf.x = fl * qd_.x; qf.y = fl * qd_.y; qf.z = fl * qd_.z;
  M3 Ro = quat_to_mat(oq.w, oq.x, oq.y, oq.z);
  V3 up = Ro.c2;
  const int j1 = limb, j2 = 4 + 2 * limb, j3 = 5 + 2 * limb;
  float* ob = sObs + envl * NO; float* st = sSt + envl * 93;
  if (limb == 0) {
    ob[0] = C.s_pos * opos.x; ob[1] = C.s_pos * opos.y; ob[2] = C.s_pos * opos.z;
    ob[3] = up.x; ob[4] = up.y; ob[5] = up.z;
    ob[6] = qf.w; ob[7] = qf.x; ob[8] = qf.y; ob[9] = qf.z;
    ob[10] = C.s_lin * olin.x; ob[11] = C.s_lin * olin.y; ob[12] = C.s_lin * olin.z;
    ob[13] = C.s_ang * oang.x; ob[14] = C.s_ang * oang.y; ob[15] = C.s_ang * oang.z;
    st[0] = C.s_pos * opos.x; st[1] = C.s_pos * opos.y; st[2] = C.s_pos * opos.z;
    st[3] = C.s_lin * olin.x; st[4] = C.s_lin * olin.y; st[5] = C.s_lin * olin.z;
    st[6] = oq.w; st[7] = oq.x; st[8] = oq.y; st[9] = oq.z;
    st[10] = C.s_ang * oang.x; st[11] = C.s_ang * oang.y; st[12] = C.s_ang * oang.z;
    st[37] = S.goal.w; st[38] = S.goal.x; st[39] = S.goal.y; st[40] = S.goal.z;
    st[41] = qf.w; st[42] = qf.x; st[43] = qf.y; st[44] = qf.z;
  }
  const int jj[3] = {j1, j2, j3};
#pragma unroll
  for (int a = 0; a < 3; a++) {
    int j = jj[a];
    ob[16 + j] = C.s_q * I.q[a]; ob[28 + j] = C.s_qd * I.qd[a]; ob[40 + j] = var2 ? 0.3f * I.tgtq[a] : I.act[a]; ob[52 + j] = var2 ? 0.3f * S.ltgt[a] : S.lact[a];      // position-control tasks: targets replace the actions (…position_control.py:438-453)
    st[13 + j] = C.s_q * I.q[a]; st[25 + j] = C.s_qd * I.qd[a]; st[69 + j] = I.act[a]; st[81 + j] = S.lact[a];
    if (var1) { ob[64 + j] = 0.3f * I.tgtq[a]; ob[76 + j] = 0.3f * S.ltgt[a]; }      // :432-455
  }
  st[45 + 3 * limb] = btip.x; st[46 + 3 * limb] = btip.y; st[47 + 3 * limb] = btip.z;
  st[57 + 3 * limb] = S.ltip.x; st[58 + 3 * limb] = S.ltip.y; st[59 + 3 * limb] = S.ltip.z;
  S.ltip = btip;
  // ---- calculate_metrics
  float vn = fminf(sqrtf(qd_.x * qd_.x + qd_.y * qd_.y + qd_.z * qd_.z), 1.0f);
  float rot_dist = 2.0f * asinf(vn);
  float rot_rew = C.quat_scale / (fabsf(rot_dist) + C.rot_eps);
  float trans = sqrtf(opos.x * opos.x + opos.y * opos.y) * C.trans_scale;
  float accp = quad_sum(fabsf(I.acc[0]) * C.acc_scale + fabsf(I.acc[1]) * C.acc_scale + fabsf(I.acc[2]) * C.acc_scale);
  float rate = quad_sum(var1 ? (fabsf(I.act[0]) + fabsf(I.act[1]) + fabsf(I.act[2]))
                             : (fabsf(S.lact[0] - I.act[0]) + fabsf(S.lact[1] - I.act[1]) + fabsf(S.lact[2] - I.act[2]))) * C.rate_scale;
  float powp = 0.f, terr = 0.f, rdec = 0.f;
  if (var1) {      // mechanical power, position-target error, rot-dist-decreasing terms (:530-545)
    powp = quad_sum(fabsf(I.torque[0] * I.qd[0]) + fabsf(I.torque[1] * I.qd[1]) + fabsf(I.torque[2] * I.qd[2])) * P->power_scale;
    terr = quad_sum(fabsf(S.ltgt[0] - I.q[0]) + fabsf(S.ltgt[1] - I.q[1]) + fabsf(S.ltgt[2] - I.q[2])) * P->target_err_scale;
    rdec = ((rot_dist > P->rot_dec_thresh) ? 1.f : 0.f) * (S.lrd - rot_dist) * P->rot_dec_scale;
    S.lrd = rot_dist;
  }
  int cgr = (S.consec > C.max_consec) ? 1 : 0;
  float bonus = C.bonus * (float)cgr;
  int succ = (fabsf(rot_dist) <= C.succ_thresh) ? 1 : 0;
  float dd = fabsf(I.q[2] - I.q[1]);
  int brk = (int)((dd < C.d23_pen[0]) | (dd > C.d23_pen[1])) + (int)((I.q[0] < C.d1_pen[0]) | (I.q[0] > C.d1_pen[1]));
  int rst = (int)((dd < C.d23_rst[0]) | (dd > C.d23_rst[1])) + (int)((I.q[0] < C.d1_rst[0]) | (I.q[0] > C.d1_rst[1]));
  brk = quad_sum_i(brk); rst = quad_sum_i(rst);
  float limp = (brk > 0) ? C.limit_pen : 0.f;
  float total = rot_rew + trans + accp + rate + bonus + limp + powp + terr + rdec;
  S.greset = cgr;
  int both = (succ && S.succ) ? 1 : 0;
  int consec = both ? (S.consec + 1) : 0;
  if (S.succ == 0 && succ == 1) consec = 1;
  S.consec = consec; S.succ = succ;
#pragma unroll
  for (int a = 0; a < 3; a++) S.lact[a] = I.act[a];
  // ---- is_done
  int reset = S.reset;
  if (opos.z > 0.f) reset = 1;
  M3 Rp; V3 pp;
  if (MODE == 0) { Rp.c0 = v3(1, 0, 0); Rp.c1 = v3(0, 1, 0); Rp.c2 = v3(0, 0, 1); pp = v3(0, 0, 0); }
  else { Rp = quat_to_mat(I.fq.w, I.fq.x, I.fq.y, I.fq.z); pp = I.fp; }
  if (mulT(Rp, pr - pp).z <= C.h_base) reset = 1;
  V3 cw = pr + mul(Rr, v3(C.corner[0], C.corner[1], C.corner[2]));
  int nlow = (mulT(Rp, cw - pp).z < C.h_corner) ? 1 : 0;
  nlow += (mulT(Rp, I.knee2 - pp).z - C.h_knee <= 0.f) ? 1 : 0;
  nlow += (mulT(Rp, I.knee3 - pp).z - C.h_knee <= 0.f) ? 1 : 0;
  nlow = quad_sum_i(nlow);
  if (nlow > 0) reset = 1;
  if (rst > 0) reset = 1;
  float fallp = C.fall_pen * (float)reset;
  total += fallp;
  if (cgr == 1) reset = 1;
  if (S.progress >= C.max_episode - 1) reset = 1;
  S.reset = reset;
  O.rew = total;
  O.terms[0] = rot_rew; O.terms[1] = trans; O.terms[2] = accp; O.terms[3] = rate; O.terms[4] = bonus; O.terms[5] = limp; O.terms[6] = fallp; O.terms[7] = (float)cgr;
  O.terms[8] = powp; O.terms[9] = terr; O.terms[10] = rdec;
  if (pd && P->cc_update_last_tgt) { S.ltgt[0] = I.tgtq[0]; S.ltgt[1] = I.tgtq[1]; S.ltgt[2] = I.tgtq[2]; }      // :723-725
}

// Which 16 envs a workgroup takes.  Workgroups go round-robin to the 8 XCDs, each with its own L2, and one row of the SoA state is 64 bytes
// per wavefront: with the identity map the two wavefronts that share a 128-byte line sit on different XCDs and both L2s fetch the whole
// line (FETCH_SIZE showed 1.8x the bytes read; tools/microbench/fetch_calib.hip reproduces the 2x with 64-byte rows).  Within each group
// of 16 workgroups the map puts blocks 2j and 2j+1 of envs on XCD j; the tail of a grid that is no multiple of 16 keeps the identity.
LM_DEV int lm_block() {
  const int b = (int)blockIdx.x;
  return b < ((int)gridDim.x & ~15) ? ((b & ~15) | ((b & 7) << 1) | ((b >> 3) & 1)) : b;
}

// shared tail: write staged obs / states, reward, counters, per-block partial sums
LM_DEV float clampf(float x, float c) { return fminf(fmaxf(x, -c), c); }

struct OutPtrs { float *obs_buf, *states_buf, *rew_buf, *terms; float *out_obs, *out_states, *out_rew; int64_t* out_resets;
                 long long* acc;          // int64 [16 + acc_rows*16]: row 0 = totals of a launch, rows 1.. = the spread first-level rows (write_outputs);
                                          // the persistent rollout (DEFER) points it at one plain row of 14 fixed-point sums per step
                 char* stats; float* extras; float* out_extras; int split_block; int acc_rows; };
#ifndef LM_ACC_COPIES
#define LM_ACC_COPIES 32         // least number of first-level accumulator rows (lm_create doubles it until a row takes < 4096 wavefronts)
#endif
#define ACC_SCALE 1048576.0f      // 2^20: integer accumulation makes the means independent of the arrival order (bitwise reproducible)
// Counted accumulator words (k_step): bits 0..11 count the arrivals, bits 12..63 hold the sum - a signed 2^20 fixed-point value for the
// reward-term means (words 0..6, 9..11), two unsigned 26-bit counts (goal resets | resets) for the success-rate windows (word 7 all envs,
// 8 first task, 12 second task).  The count never carries into the sum: a word sees at most 4095 arrivals.
#define ACC_CNT_BITS 12
#define ACC_CNT_MASK 4095LL
#define ACC_WIN_BITS 26

LM_DEV void success_window(int64_t* ns, float* rate, int64_t add_succ, int64_t add_rst, int64_t max_cnt) {
  int64_t num_succ = ns[0], num_rst = ns[1]; float sr = *rate;
  if (num_rst > max_cnt) { sr = (float)num_succ / (float)num_rst; num_rst = 0; num_succ = 0; }
  ns[0] = num_succ + add_succ; ns[1] = num_rst + add_rst; *rate = sr;
}

// The lane that completed word k of a launch publishes what depends on it: a mean of a reward term, or one success-rate window
// (quadruped_pose_control.py:560,610,618-633; the co-train task keeps two more windows for its halves, joint_locomanipulation.py:795-859).
// The 13 words are independent of each other, so their last arrivals may be lanes of different wavefronts.
LM_DEV void publish_extra(const lm_params* __restrict__ P, const OutPtrs& W, int N, int k, long long tot) {
  if (k == 7 || k == 8 || k == 12) {
    const int w = (k == 7) ? 0 : (k == 8) ? 1 : 2;
    int64_t* ns = reinterpret_cast<int64_t*>(W.stats); float* rate = reinterpret_cast<float*>(W.stats + 48);
    success_window(ns + 2 * w, rate + w, (int64_t)(tot >> ACC_WIN_BITS), (int64_t)(tot & ((1LL << ACC_WIN_BITS) - 1)), (int64_t)P->max_reset_counts);
    W.extras[7 + w] = rate[w]; if (W.out_extras) W.out_extras[7 + w] = rate[w];
  } else {
    const float m = (float)((double)tot * (1.0 / (double)ACC_SCALE)) / (float)N;
    const int e = (k < 7) ? k : k + 1;      // words 9..11 are extras 10..12
    W.extras[e] = m; if (W.out_extras) W.out_extras[e] = m;
  }
}

struct DrOut { int64_t* drc; uint32_t seed, dr_step; int64_t rand_buf, reset_key; uint32_t* sKey; };      // sKey: LDS [16][2] {corr key, fire}

#ifdef LM_HELPER_WAVE
// Whether a wavefront's outputs go out as whole float4 blocks: 16 envs and a 16-byte aligned out_states.  Wave-uniform, from kernel arguments only
LM_DEV bool outputs_full(const OutPtrs& W, int N, int env0) {
  return (min(ENVS_PER_WAVE, N - env0) == ENVS_PER_WAVE) && (reinterpret_cast<uintptr_t>(W.out_states) & 15) == 0;
}
// k_step_h3 (OW): the staged obs and states of a full wavefront without observation noise leave on the terms helper wavefront, behind the one
// workgroup barrier wavefront 0 passes where write_outputs has its staging wait.  The loop is write_outputs' full-wavefront streaming path:
// plain copies and clamps of what wavefront 0 staged in LDS, so the same bits.  Otherwise the helper only passes the barrier
template <int NB>
LM_DEV void helper_write_outputs(const lm_params* __restrict__ P, const OutPtrs& W, int N, int env0, int lane, const float* sObs, const float* sSt) {
  hw_barrier();      // wavefront 0's staging writes are in LDS
  if (!outputs_full(W, N, env0)) return;
  const float clip = P->clip_obs;
  auto clamp4 = [&](float4 v) { v.x = clampf(v.x, clip); v.y = clampf(v.y, clip); v.z = clampf(v.z, clip); v.w = clampf(v.w, clip); return v; };
  constexpr int NV = ENVS_PER_WAVE * NB / 4, NS = ENVS_PER_WAVE * 93 / 4, KV = (NV + 63) / 64, KS = (NS + 63) / 64;
  float4 vo[KV], vs[KS];
#pragma unroll
  for (int k = 0; k < KV; k++) { const int i = lane + 64 * k; vo[k] = reinterpret_cast<const float4*>(sObs)[(NV % 64 == 0 || i < NV) ? i : 0]; }
#pragma unroll
  for (int k = 0; k < KS; k++) { const int i = lane + 64 * k; vs[k] = reinterpret_cast<const float4*>(sSt)[(NS % 64 == 0 || i < NS) ? i : 0]; }
  float4* ob = reinterpret_cast<float4*>(W.obs_buf + (size_t)env0 * NB); float4* oo = reinterpret_cast<float4*>(W.out_obs + (size_t)env0 * NB);
  float4* sb = reinterpret_cast<float4*>(W.states_buf + (size_t)env0 * 93); float4* so = reinterpret_cast<float4*>(W.out_states + (size_t)env0 * 93);
  if (W.out_obs) {
#pragma unroll
    for (int k = 0; k < KV; k++) { const int i = lane + 64 * k; if (NV % 64 == 0 || i < NV) oo[i] = clamp4(vo[k]); }
  }
  if (W.out_states) {
#pragma unroll
    for (int k = 0; k < KS; k++) { const int i = lane + 64 * k; if (NS % 64 == 0 || i < NS) so[i] = clamp4(vs[k]); }
  }
  if (W.obs_buf) {
#pragma unroll
    for (int k = 0; k < KV; k++) { const int i = lane + 64 * k; if (NV % 64 == 0 || i < NV) ob[i] = vo[k]; }
  }
  if (W.states_buf) {
#pragma unroll
    for (int k = 0; k < KS; k++) { const int i = lane + 64 * k; if (NS % 64 == 0 || i < NS) sb[i] = vs[k]; }
  }
}
#endif

// OW 1 (wavefront 0 of k_step_h3): the staging wait is a workgroup barrier, and the full-wavefront streaming loop runs on the terms helper
// wavefront (helper_write_outputs)
template <int DR, int DEFER = 0, int NOBS = 0, int OW = 0>      // DEFER 1: only accumulate; the extras of this step are published later (persistent rollout kernel); NOBS 0: width from the parameters
LM_DEV void write_outputs(const lm_params* __restrict__ P, const OutPtrs& W, int N, int env0, int lane, int limb, int env, bool active,
                          const TaskState& S, const TaskOut& O, int64_t* cnt, int episode, float* sObs, float* sSt, const DrOut& DO) {
  if (DR) {
    // observation-noise bookkeeping with the flags is_done has just written (vec_env_rlgames.py:70-72; randomize.py:213-216,228-230)
    int64_t oc = S.reset ? 0 : DO.drc[0 * (size_t)N + env];
    oc += 1;
    const lm_dr_channel& ci = P->dr[LM_DR_OBS_INTERVAL];
    const bool fire = ci.enabled && oc >= ci.interval;
    if (fire) oc = 0;
    if (limb == 0) { DO.sKey[2 * (lane >> 2)] = (uint32_t)episode + (S.reset ? 1u : 0u); DO.sKey[2 * (lane >> 2) + 1] = fire ? 1u : 0u; }
    if (active && limb == 0) {
      DO.drc[0 * (size_t)N + env] = oc; DO.drc[2 * (size_t)N + env] = (int64_t)DO.dr_step + 1;
      DO.drc[3 * (size_t)N + env] = DO.rand_buf + 1; DO.drc[4 * (size_t)N + env] = DO.reset_key;
    }
  }
#ifdef LM_HELPER_WAVE
  if (OW) hw_barrier();      // the staging writes landed, and the helper wavefront that streams them out may start
  else
#endif
  {
  __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): LDS staging writes landed (single wave per block)
  __builtin_amdgcn_wave_barrier();
  }
  // per-block partial sums in a fixed order (deterministic means).  Every lane of a quad holds its env's terms; lane 3 is the one that counts
  float tot0[12];
  {
    const bool cnts = active && (limb == 3);
#pragma unroll
    for (int k = 0; k < 8; k++) tot0[k] = wave_sum_lane3(cnts ? O.terms[k] : 0.f);
    tot0[8] = wave_sum_lane3(cnts ? (float)S.reset : 0.f);
#pragma unroll
    for (int k = 0; k < 3; k++) tot0[9 + k] = wave_sum_lane3(cnts ? O.terms[8 + k] : 0.f);
  }
  // ---- means of the reward terms + success-rate windows.  Every wavefront adds its partial sums to a first-level row (row = block index
  // mod acc_rows, so that 256 wavefronts do not serialise on one cache line) with ONE returning device-scope atomic per word; the word
  // counts its arrivals, so the lane whose add completes a row's word knows it holds the row's total, adds that to the launch's word
  // (row 0) the same way, and the lane that completes that one publishes the extras entry: two dependent round trips on the critical
  // path, no ticket, no read-back, and every word is left zero for the next launch.  Integer sums: the totals do not depend on the order.
  long long acc_old = 0, acc_add = 0;
  long long* acc_row = W.acc;
  {
    const bool first_task = lm_block() < W.split_block;
    float mine = 0.f;
#pragma unroll
    for (int k = 0; k < 12; k++) mine = (lane == k) ? tot0[k] : mine;
    if (DEFER) {      // per-step rows of the persistent rollout kernel: 14 plain fixed-point sums, read by k_rollout_finalize
      mine = (lane == 12) ? (first_task ? tot0[7] : 0.f) : mine;
      mine = (lane == 13) ? (first_task ? tot0[8] : 0.f) : mine;
      if (lane < 14) acc_old = __hip_atomic_fetch_add(acc_row + lane, (long long)llrintf(mine * ACC_SCALE), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      const long long win = ((long long)llrintf(tot0[7]) << ACC_WIN_BITS) + (long long)llrintf(tot0[8]);      // (goal resets | resets) of these 16 envs
      long long c = (long long)llrintf(mine * ACC_SCALE);
      c = (lane == 7) ? win : c;
      c = (lane == 8) ? (first_task ? win : 0LL) : c;
      c = (lane == 12) ? (first_task ? 0LL : win) : c;
      acc_add = c * (1LL << ACC_CNT_BITS) + 1LL;
      acc_row = W.acc + 16 + (size_t)((int)blockIdx.x & (W.acc_rows - 1)) * 16;
      if (lane < 13) acc_old = __hip_atomic_fetch_add(acc_row + lane, acc_add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  const float clip = P->clip_obs;
  int nenv = min(ENVS_PER_WAVE, N - env0);
  const int NO = NOBS ? NOBS : P->num_obs;
  auto clamp4 = [&](float4 v) { v.x = clampf(v.x, clip); v.y = clampf(v.y, clip); v.z = clampf(v.z, clip); v.w = clampf(v.w, clip); return v; };
  const bool full = (nenv == ENVS_PER_WAVE) && (reinterpret_cast<uintptr_t>(W.out_states) & 15) == 0;
  if (OW && !DR && NOBS && full) {
    // (k_step_h3: the terms helper wavefront streams the staging out, helper_write_outputs)
  } else if (!DR && NOBS && full) {
    // a full wavefront without observation noise: 16 rows of obs (NOBS floats, a multiple of 4) and of states (93 floats; env0 is a multiple
    // of 16: 5952-byte offsets) are contiguous blocks of float4.  Known trip counts: all LDS reads are issued before the first store
    constexpr int NB = NOBS ? NOBS : 64, NV = ENVS_PER_WAVE * NB / 4, NS = ENVS_PER_WAVE * 93 / 4, KV = (NV + 63) / 64, KS = (NS + 63) / 64;
    float4 vo[KV], vs[KS];
#pragma unroll
    for (int k = 0; k < KV; k++) { const int i = lane + 64 * k; vo[k] = reinterpret_cast<const float4*>(sObs)[(NV % 64 == 0 || i < NV) ? i : 0]; }
#pragma unroll
    for (int k = 0; k < KS; k++) { const int i = lane + 64 * k; vs[k] = reinterpret_cast<const float4*>(sSt)[(NS % 64 == 0 || i < NS) ? i : 0]; }
    float4* ob = reinterpret_cast<float4*>(W.obs_buf + (size_t)env0 * NB); float4* oo = reinterpret_cast<float4*>(W.out_obs + (size_t)env0 * NB);
    float4* sb = reinterpret_cast<float4*>(W.states_buf + (size_t)env0 * 93); float4* so = reinterpret_cast<float4*>(W.out_states + (size_t)env0 * 93);
    if (W.out_obs) {
#pragma unroll
      for (int k = 0; k < KV; k++) { const int i = lane + 64 * k; if (NV % 64 == 0 || i < NV) oo[i] = clamp4(vo[k]); }
    }
    if (W.out_states) {
#pragma unroll
      for (int k = 0; k < KS; k++) { const int i = lane + 64 * k; if (NS % 64 == 0 || i < NS) so[i] = clamp4(vs[k]); }
    }
    if (W.obs_buf) {
#pragma unroll
      for (int k = 0; k < KV; k++) { const int i = lane + 64 * k; if (NV % 64 == 0 || i < NV) ob[i] = vo[k]; }
    }
    if (W.states_buf) {
#pragma unroll
      for (int k = 0; k < KS; k++) { const int i = lane + 64 * k; if (NS % 64 == 0 || i < NS) sb[i] = vs[k]; }
    }
  } else {
  // obs: nenv*NO floats contiguous (NO = 64 or 88, both multiples of 4)
  for (int i = lane; i < nenv * (NO / 4); i += 64) {
    float4 v = reinterpret_cast<const float4*>(sObs)[i];
    if (DR) {      // noise in place on obs_buf, then the clipObservations clamp on the returned copy
      const int el = (4 * i) / NO, col = (4 * i) - el * NO;
      const uint32_t ckey = DO.sKey[2 * el], fire = DO.sKey[2 * el + 1], e = (uint32_t)(env0 + el);
      const lm_dr_channel& cr = P->dr[LM_DR_OBS_RESET]; const lm_dr_channel& ci = P->dr[LM_DR_OBS_INTERVAL];
      float x[4] = {v.x, v.y, v.z, v.w};
      const uint32_t cpair = (uint32_t)col >> 1;          // col is a multiple of 4: components (col, col+1) and (col+2, col+3) are Box-Muller pairs
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if (cr.enabled) x[k] = dr_apply(cr.operation, x[k], dr_sample(DO.seed, LM_DR_OBS_RESET, e, ckey, 2u * cpair + (uint32_t)k, cr.distribution, cr.p0[0], cr.p1[0]));
        if (fire) x[k] = dr_apply(ci.operation, x[k], dr_sample(DO.seed, LM_DR_OBS_INTERVAL, e, DO.dr_step, 2u * cpair + (uint32_t)k, ci.distribution, ci.p0[0], ci.p1[0]));
      }
      v.x = x[0]; v.y = x[1]; v.z = x[2]; v.w = x[3];
    }
    if (W.obs_buf) reinterpret_cast<float4*>(W.obs_buf + (size_t)env0 * NO)[i] = v;
    if (W.out_obs) reinterpret_cast<float4*>(W.out_obs + (size_t)env0 * NO)[i] = clamp4(v);
  }
  // states: 16 rows of 93 floats are one contiguous block of 372 float4 (env0 is a multiple of 16: 5952-byte offsets)
  if (full) {
    for (int i = lane; i < ENVS_PER_WAVE * 93 / 4; i += 64) {
      float4 v = reinterpret_cast<const float4*>(sSt)[i];
      if (W.states_buf) reinterpret_cast<float4*>(W.states_buf + (size_t)env0 * 93)[i] = v;
      if (W.out_states) reinterpret_cast<float4*>(W.out_states + (size_t)env0 * 93)[i] = clamp4(v);
    }
  } else {
    for (int i = lane; i < nenv * 93; i += 64) {
      float v = sSt[i];
      if (W.states_buf) W.states_buf[(size_t)env0 * 93 + i] = v;
      if (W.out_states) W.out_states[(size_t)env0 * 93 + i] = clampf(v, clip);
    }
  }
  }
  if (active && limb == 0) {
    W.rew_buf[env] = O.rew;
    if (W.out_rew) W.out_rew[env] = O.rew;
    if (W.out_resets) W.out_resets[env] = (int64_t)S.reset;
    cnt[0 * (size_t)N + env] = S.succ; cnt[1 * (size_t)N + env] = S.consec; cnt[2 * (size_t)N + env] = S.greset;
    cnt[3 * (size_t)N + env] = S.reset; cnt[4 * (size_t)N + env] = S.progress; cnt[5 * (size_t)N + env] = episode;
    if (W.terms) {
#pragma unroll
      for (int k = 0; k < 11; k++) W.terms[(size_t)k * N + env] = O.terms[k];
    }
  }
  LM_STAMP(9);      // partial sums, atomics issued, output stores issued
  if (!DEFER) {
    const int rows = W.acc_rows, r = (int)blockIdx.x & (rows - 1);
    const int in_row = ((int)gridDim.x - 1 - r) / rows + 1;      // wavefronts of this launch that add to row r
    if (lane < 13 && (int)(acc_old & ACC_CNT_MASK) == in_row - 1) {
      const long long t1 = (acc_old + acc_add) >> ACC_CNT_BITS;      // the row's total of word `lane`
      __hip_atomic_store(acc_row + lane, 0LL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const long long add2 = t1 * (1LL << ACC_CNT_BITS) + 1LL;
      const long long old2 = __hip_atomic_fetch_add(W.acc + lane, add2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((int)(old2 & ACC_CNT_MASK) == min(rows, (int)gridDim.x) - 1) {
        __hip_atomic_store(W.acc + lane, 0LL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        publish_extra(P, W, N, lane, (old2 + add2) >> ACC_CNT_BITS);
      }
    }
  } else {
    asm volatile("" :: "v"(acc_old));
  }
}
