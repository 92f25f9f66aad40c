// lm_step.h -- device code of the step, layer 4 of 4: the kernel arguments, step_body (one control step of 16 envs on one wavefront) and the
// shared-memory / stamp macros of the step kernels.
#pragma once
#include "lm_task.h"

LM_DEV void load_table(const float* __restrict__ table, float* sTab, int lane) {
  for (int i = lane; i < LM_ITAB_FLOATS; i += 64) sTab[i] = table[i];
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_wave_barrier();
}
// the same in two halves so that the table's round trip overlaps the state loads of the step kernel
#define TABLE_REGS ((LM_ITAB_FLOATS + 63) / 64)
struct TableRegs { float v[TABLE_REGS]; };
LM_DEV void table_fetch(const float* __restrict__ table, int lane, TableRegs& T) {
#pragma unroll
  for (int j = 0; j < TABLE_REGS; j++) { int i = lane + 64 * j; T.v[j] = (i < LM_ITAB_FLOATS) ? table[i] : 0.f; }
}
LM_DEV void table_commit(const TableRegs& T, float* sTab, int lane) {
#pragma unroll
  for (int j = 0; j < TABLE_REGS; j++) { int i = lane + 64 * j; if (i < LM_ITAB_FLOATS) sTab[i] = T.v[j]; }
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_wave_barrier();
}

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
struct StepArgs {
  const lm_params* params; const float* table; float* state; int64_t* cnt;
  const float* actions; const float* goal_rand; OutPtrs W; int N, split; uint32_t seed;
  int skip_reset;   // 1: leave reset_buf untouched (staged API: resets were applied by lm_apply_resets)
  int nsub;         // < 0: params.substeps, otherwise that many sub-steps (0 = read-back + task layer only)
  int64_t* drc;     // domain-randomisation counters [LM_DR_CNT_ROWS][N] (k_step_dr only)
  float* dr_phys;   // [LM_DR_PHYS_ROWS][N] attributes sampled for this step (k_step_dr only)
  int kind[2];      // variant * 2 + (mode == LM_MODE_MANI) of the two parameter blocks: the kernels pick their specialisation from the kernel
                    // arguments, so the first loads of the step do not wait for a round trip to the parameter block
  const lm_reset_dr* reset_dr;      // reset-state channels of the two blocks, followed by float [LM_DR_RESET_ROWS][N]: the state each env was last
                                    // reset to (k_step_dr / k_step_dr_pd only; kept last so that no other member moves)
  const lm_mass_dr* mass_dr;        // mass channels of the two blocks, followed by float [LM_DR_MASS_ROWS][N]: the masses the last step used
                                    // (k_step_dr / k_step_dr_pd only; appended for the same reason)
  const float* env_params;          // [LM_ENV_PARAM_ROWS][N] per-env parameters held by the caller (k_step_dr_hp / k_step_dr_pd_hp only; NULL unless lm_enable_env_params).  In the
                                    // slot that used to be reserved: the arguments that follow StepArgs (k_substeps, k_fk, k_rollout ...) keep their 16-byte phase
  float* contact;                   // [LM_CONTACT_ROWS][N] contact record (the *_cf kernels only; NULL unless reporting is on; appended for the same reason)
  const uint64_t* env_mask;         // [2] which rows of env_params are held (bit r of the 128: row r; the same kernels; the second formerly reserved slot)
  const lm_actuator_dr* actuator_dr;      // actuator channels of the two blocks, followed by float [LM_DR_ACTUATOR_ROWS][N]: kp, kd and latency the last
                                    // step used (the randomised kernels only; the new last member)
};
extern "C" __attribute__((visibility("hidden"))) void lm_internal_launch_step_w2(const StepArgs* A, int nblocks, hipStream_t s);      // k_step_w2's launcher (lm_engine_w2.hip), called by lm_step
extern "C" __attribute__((visibility("hidden"))) void lm_internal_launch_step_h2(const StepArgs* A, int nblocks, hipStream_t s);      // k_step_h2's launcher (lm_engine_h2.hip), called by lm_step
extern "C" __attribute__((visibility("hidden"))) void lm_internal_launch_step_h3(const StepArgs* A, int nblocks, hipStream_t s);      // k_step_h3's launcher (lm_engine_h3.hip), called by lm_step
extern "C" __attribute__((visibility("hidden"))) void lm_internal_launch_step_hp(const StepArgs* A, int pd, int nblocks, hipStream_t s);      // k_step_dr_hp / k_step_dr_pd_hp's launcher (lm_engine_hp.hip), called by lm_step

// The task-layer state of one lane at the start of a step: the counters and the last action / joint rate / tip / goal from memory, and for an env
// that is reset in this step the values reset_idx gives them, the new goal drawn from goal_rand or the hash, and the next episode number.  It
// depends only on what is in memory at kernel entry and on the kernel arguments.  Every step kernel runs it behind the physics (issuing the
// loads at the top of the last sub-step was measured and gains nothing); in k_step_h3 wavefront 1 runs it while wavefront 0 is in the
// second half of the last sub-step (helper_task_state)
// (a macro on the caller's own locals - st, cnt, N, env, limb, jj, do_reset, pd, MODE, A, P; S, episode, lqd - and not a function: called as a
// function from step_body it moved the instructions of the other step kernels, which tools/isa_diff.py does not allow)
#define LM_TASK_STATE_LOAD \
  S.succ = (int)cnt[0 * (size_t)N + env]; S.consec = (int)cnt[1 * (size_t)N + env]; S.greset = (int)cnt[2 * (size_t)N + env]; \
  S.reset = (int)cnt[3 * (size_t)N + env]; S.progress = (int)cnt[4 * (size_t)N + env]; episode = (int)cnt[5 * (size_t)N + env]; \
_Pragma("unroll") \
  for (int a = 0; a < 3; a++) { S.lact[a] = st[(size_t)(R_LACT + jj[a]) * N + env]; lqd[a] = st[(size_t)(R_LQD + jj[a]) * N + env]; } \
  S.ltip = v3(st[(size_t)(R_LTIP + 3 * limb) * N + env], st[(size_t)(R_LTIP + 3 * limb + 1) * N + env], st[(size_t)(R_LTIP + 3 * limb + 2) * N + env]); \
  S.goal.w = st[(size_t)(R_GOAL + 0) * N + env]; S.goal.x = st[(size_t)(R_GOAL + 1) * N + env]; S.goal.y = st[(size_t)(R_GOAL + 2) * N + env]; S.goal.z = st[(size_t)(R_GOAL + 3) * N + env]; \
  S.lrd = 0.f; S.ltgt[0] = S.ltgt[1] = S.ltgt[2] = 0.f; \
  if (pd) { \
_Pragma("unroll") \
    for (int a = 0; a < 3; a++) S.ltgt[a] = st[(size_t)(R_LTGT + jj[a]) * N + env]; \
    S.lrd = st[(size_t)R_LRD * N + env]; \
  } \
  if (do_reset) { \
    float u3[3]; \
    if (A.goal_rand) { u3[0] = A.goal_rand[(size_t)env * 3]; u3[1] = A.goal_rand[(size_t)env * 3 + 1]; u3[2] = A.goal_rand[(size_t)env * 3 + 2]; } \
    else hash_uniform3(A.seed, (uint32_t)env, (uint32_t)episode, u3); \
    S.goal = quat_from_euler(P->goal_lo[0] + (P->goal_hi[0] - P->goal_lo[0]) * u3[0], P->goal_lo[1] + (P->goal_hi[1] - P->goal_lo[1]) * u3[1], \
                             P->goal_lo[2] + (P->goal_hi[2] - P->goal_lo[2]) * u3[2]); \
_Pragma("unroll") \
    for (int a = 0; a < 3; a++) { S.lact[a] = 0.f; lqd[a] = 0.f; } \
    S.ltip = v3(P->default_tip[3 * limb], P->default_tip[3 * limb + 1], P->default_tip[3 * limb + 2]); \
    S.succ = 0; S.consec = 0; S.greset = 0; S.reset = 0; S.progress = 0; episode += 1; \
    if (pd) { \
_Pragma("unroll") \
      for (int a = 0; a < 3; a++) S.ltgt[a] = P->init_q[jj[a]]; \
      Q4 qb; qb.w = (MODE == 0) ? P->init_base_quat[0] : 1.f; qb.x = (MODE == 0) ? -P->init_base_quat[1] : 0.f; \
      qb.y = (MODE == 0) ? -P->init_base_quat[2] : 0.f; qb.z = (MODE == 0) ? -P->init_base_quat[3] : 0.f; \
      Q4 d4 = qmul(qb, qconj(S.goal)); \
      S.lrd = 2.0f * asinf(fminf(sqrtf(d4.x * d4.x + d4.y * d4.y + d4.z * d4.z), 1.0f)); \
    } \
  }
template <int MODE, int VAR>
LM_DEV void task_state_load(const StepArgs& A, const lm_params* __restrict__ P, float* st, int64_t* cnt, int N, int env, int limb, const int (&jj)[3],
                            bool do_reset, TaskState& S, int& episode, float (&lqd)[3]) {
  constexpr bool pd = (VAR >= 1);
  LM_TASK_STATE_LOAD
}

// REG0: substep()'s first drive pass runs on registers (1, the step kernels) or reads the stash back like the second (0: k_step_w2 and the
// persistent rollouts, whose register budget has no room for it; same arithmetic, same bits)
// HW: wavefront 0 of k_step_h2, whose helper wavefront computes the limb bias terms of every sub-step (helper_wave, lm_dynamics.h)
// (HW 2: wavefront 0 of k_step_h3, whose second helper computes the contact terms too: helper_wave_terms.)  OW: that helper also streams the
// staged obs / states of a full wavefront out (write_outputs, helper_write_outputs)
// HP: the randomised step of an engine with caller-held per-env parameters (lm_enable_env_params; k_step_dr_hp / k_step_dr_pd_hp, DR = 1 only): the
// value of every held row of A.env_params replaces what the channels produced, before the record rows are written.  The mask is wave-uniform
// TS (wavefront 0 of k_step_h3 only, HW 2; LM_H3_TAIL_STATE): the task-layer state comes from LDS, where wavefront 1 put it during the last
// sub-step (helper_task_state)
template <int MODE, int VAR, int DR, int DEFER = 0, int CF = 0, int REG0 = 1, int HW = 0, int OW = 0, int HP = 0, int TS = 0>
LM_DEV void step_body(const StepArgs& A, const lm_params* __restrict__ P, float* sTab, float* sObs, float* sSt, float4* sStash) {
  TableRegs TR; table_fetch(A.table, threadIdx.x, TR);
  const int lane = threadIdx.x, limb = lane & 3, envl = lane >> 2;
  const int env0 = lm_block() * ENVS_PER_WAVE, envr = env0 + envl, N = A.N;
  const bool active = envr < N; const int env = active ? envr : (N - 1);
  const float* tl = sTab + HUB_FLOATS + limb * LIMB_STRIDE;
  const int jj[3] = {limb, 4 + 2 * limb, 5 + 2 * limb};
  float* st = A.state; int64_t* cnt = A.cnt;
  const int fb = (MODE == 0) ? R_FB0 : R_FB1;
  Stash St; St.base = sStash; St.lane = lane;
  // ---- load the physical state (the task-layer state is loaded after the physics to keep registers free)
  const bool do_reset = (cnt[3 * (size_t)N + env] != 0) && !A.skip_reset;
  FreeBody F; V3 lin, ang; float q[3], qd[3], act[3];
  F.p = v3(st[(size_t)(fb + 0) * N + env], st[(size_t)(fb + 1) * N + env], st[(size_t)(fb + 2) * N + env]);
  F.q.w = st[(size_t)(fb + 3) * N + env]; F.q.x = st[(size_t)(fb + 4) * N + env]; F.q.y = st[(size_t)(fb + 5) * N + env]; F.q.z = st[(size_t)(fb + 6) * N + env];
  lin = v3(st[(size_t)(fb + 7) * N + env], st[(size_t)(fb + 8) * N + env], st[(size_t)(fb + 9) * N + env]);
  ang = v3(st[(size_t)(fb + 10) * N + env], st[(size_t)(fb + 11) * N + env], st[(size_t)(fb + 12) * N + env]);
#pragma unroll
  for (int a = 0; a < 3; a++) {
    q[a] = st[(size_t)(R_Q + jj[a]) * N + env]; qd[a] = st[(size_t)(R_QD + jj[a]) * N + env];
    act[a] = A.actions[(size_t)env * 12 + jj[a]];
  }
  DrPhys X; uint32_t dr_step = 0; int64_t dr_rand_buf = 0, dr_reset_key = 0; bool reset_draw = false;
  // HP: the row mask (bits 0..63, 64..68) and the table; held(r) may be lane-dependent through r, the mask itself is not
  const uint64_t hp_lo = HP ? A.env_mask[0] : 0ull; const uint32_t hp_hi = HP ? (uint32_t)A.env_mask[1] : 0u; const float* hp = A.env_params;
  const auto held = [&](int r) -> bool { return HP && (r < 64 ? (hp_lo >> r) & 1ull : (uint64_t)(hp_hi >> (r - 64)) & 1ull) != 0; };
  const auto held_value = [&](int r, float x) -> float { return held(r) ? hp[(size_t)r * N + env] : x; };
  if (DR) {
    // ---- action noise on the raw actions (vec_env_rlgames.py:56-58; randomize.py:237-259): correlated noise keyed by the episode this
    // step belongs to (redrawn exactly when the reset flag is set), uncorrelated noise every frequency_interval calls
    int64_t* dc = A.drc;
    const uint32_t ep_now = (uint32_t)cnt[5 * (size_t)N + env] + (do_reset ? 1u : 0u);
    dr_step = (uint32_t)dc[2 * (size_t)N + env]; dr_rand_buf = dc[3 * (size_t)N + env]; dr_reset_key = dc[4 * (size_t)N + env];
    int64_t ac = do_reset ? 0 : dc[1 * (size_t)N + env];
    ac += 1;
    const lm_dr_channel& cr = P->dr[LM_DR_ACT_RESET]; const lm_dr_channel& ci = P->dr[LM_DR_ACT_INTERVAL];
    const bool fire = ci.enabled && ac >= ci.interval;
    if (fire) ac = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      if (cr.enabled) act[a] = dr_apply(cr.operation, act[a], dr_sample(A.seed, LM_DR_ACT_RESET, (uint32_t)env, ep_now, (uint32_t)jj[a], cr.distribution, cr.p0[0], cr.p1[0]));
      if (fire) act[a] = dr_apply(ci.operation, act[a], dr_sample(A.seed, LM_DR_ACT_INTERVAL, (uint32_t)env, dr_step, (uint32_t)jj[a], ci.distribution, ci.p0[0], ci.p1[0]));
    }
    if (active && limb == 0) dc[1 * (size_t)N + env] = ac;
    // ---- gated on_reset randomisation (quadruped_pose_control.py:224-228), then this control step's physics attributes
    reset_draw = do_reset && dr_rand_buf >= P->dr_min_frequency;
    if (reset_draw) { dr_reset_key = ep_now; dr_rand_buf = 0; }
    const float g0[3] = {0.f, 0.f, -P->gravity}; float gv[3], fv[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      gv[c] = dr_attr(P->dr[LM_DR_GRAVITY], A.seed, LM_DR_GRAVITY, env, dr_step, (uint32_t)dr_reset_key, c, c, g0[c]);
      fv[c] = dr_attr(P->dr[LM_DR_BASE_FORCE], A.seed, LM_DR_BASE_FORCE, env, dr_step, (uint32_t)dr_reset_key, c, c, 0.f);
      X.tmax[c] = dr_attr(P->dr[LM_DR_MAX_EFFORT], A.seed, LM_DR_MAX_EFFORT, env, dr_step, (uint32_t)dr_reset_key, jj[c], 0, P->tau_max);
      X.vmax[c] = dr_attr(P->dr[LM_DR_MAX_VELOCITY], A.seed, LM_DR_MAX_VELOCITY, env, dr_step, (uint32_t)dr_reset_key, jj[c], 0, P->max_joint_vel);
      X.cj[c] = dr_attr(P->dr[LM_DR_JOINT_DAMPING], A.seed, LM_DR_JOINT_DAMPING, env, dr_step, (uint32_t)dr_reset_key, jj[c], 0, P->joint_damping);
    }
    if (HP) {      // rows of LM_PTR_DR_PHYS: max efforts 0, max joint velocities 12, gravity 24, base force 27, joint damping 30
#pragma unroll
      for (int c = 0; c < 3; c++) {
        X.tmax[c] = held_value(jj[c], X.tmax[c]); X.vmax[c] = held_value(12 + jj[c], X.vmax[c]); X.cj[c] = held_value(30 + jj[c], X.cj[c]);
        gv[c] = held_value(24 + c, gv[c]); fv[c] = held_value(27 + c, fv[c]);
      }
    }
    X.g = v3(gv[0], gv[1], gv[2]); X.f = v3(fv[0], fv[1], fv[2]);
    // contact material: mu_env = friction_scale x combine(feet, ground / plate); the block's mu when neither channel is on
    const lm_dr_channel& mr = P->dr_mat[LM_DR_MAT_ROBOT]; const lm_dr_channel& mo = P->dr_mat[LM_DR_MAT_OTHER];
    X.mu = P->mu;
    if (mr.enabled || mo.enabled) {
      const float fr = dr_material(mr, P->dr_mat_buckets[LM_DR_MAT_ROBOT], A.seed, LM_DR_STREAM_MAT + LM_DR_MAT_ROBOT, env, dr_step, (uint32_t)dr_reset_key, P->mat_mu_robot);
      const float fo = dr_material(mo, P->dr_mat_buckets[LM_DR_MAT_OTHER], A.seed, LM_DR_STREAM_MAT + LM_DR_MAT_OTHER, env, dr_step, (uint32_t)dr_reset_key, P->mat_mu_other);
      X.mu = fmaxf(P->friction_scale * friction_combine(P->friction_combine, fr, fo), 0.f);
    }
    if (HP) X.mu = held_value(LM_DR_PHYS_MU, X.mu);      // mu_env itself: after friction_scale and the combine mode
    // mass channels: this lane's five limb bodies, the hub and, in a manipulation block, the plate.  The switches are
    // wave-uniform (one parameter block per wavefront): with all channels off nothing below runs and the sub-steps take the table's path
    {
      const lm_mass_dr* MD = A.mass_dr + ((env0 >= A.split) ? 1 : 0);
      const lm_dr_channel& cb = MD->ch[LM_DR_MASS_BODIES];
      X.mb_on = cb.enabled;
      X.mp_on = (MODE == 1 && (MD->ch[LM_DR_MASS_PLATE].enabled || MD->ch[LM_DR_MASS_PLATE_DENSITY].enabled)) ? 1 : 0;
      if (HP) {      // rows LM_DR_PHYS_ROWS + (plate mass 0, plate inertia factor 1, body masses 2..22): a held row switches its path on, as its channel does
        if ((hp_lo >> (LM_DR_PHYS_ROWS + 2)) != 0ull || (hp_hi & 3u) != 0u) X.mb_on = 1;
        if (MODE == 1 && ((hp_lo >> LM_DR_PHYS_ROWS) & 3ull) != 0ull) X.mp_on = 1;
      }
      float* mrec = (float*)(A.mass_dr + 2);
      if (X.mb_on) {
        const float* tn = A.table + HUB_FLOATS + limb * LIMB_STRIDE;      // nominal masses: the device table in memory (LDS is not filled yet)
        const float nom[5] = {tn[T_I0], tn[T_Q1], tn[T_Q2], tn[T_Q1 + 1], tn[T_Q2 + 1]};      // shell, link4, link3, link1, link2
        const int c0 = 1 + 5 * limb; float mm[5];
#pragma unroll
        for (int j = 0; j < 5; j++)
          mm[j] = dr_mass(cb, A.seed, LM_DR_STREAM_MASS + LM_DR_MASS_BODIES, env, dr_step, (uint32_t)dr_reset_key, (uint32_t)(c0 + j), MD->body_p0[c0 + j], MD->body_p1[c0 + j], nom[j]);
        if (HP) {
#pragma unroll
          for (int j = 0; j < 5; j++) mm[j] = held_value(LM_DR_PHYS_ROWS + 2 + c0 + j, mm[j]);
        }
        X.m_s = mm[0]; X.m_41 = mk2(mm[1], mm[3]); X.m_32 = mk2(mm[2], mm[4]);
        X.m_hub = dr_mass(cb, A.seed, LM_DR_STREAM_MASS + LM_DR_MASS_BODIES, env, dr_step, (uint32_t)dr_reset_key, 0U, MD->body_p0[0], MD->body_p1[0], A.table[0]);
        if (HP) X.m_hub = held_value(LM_DR_PHYS_ROWS + 2, X.m_hub);
        if (active) {
#pragma unroll
          for (int j = 0; j < 5; j++) mrec[(size_t)(2 + c0 + j) * N + env] = mm[j];
          if (limb == 0) mrec[(size_t)2 * N + env] = X.m_hub;
        }
      }
      if (MODE == 1 && X.mp_on) {
        const lm_dr_channel& cm = MD->ch[LM_DR_MASS_PLATE]; const lm_dr_channel& cd = MD->ch[LM_DR_MASS_PLATE_DENSITY];
        X.s_plate = dr_mass(cd, A.seed, LM_DR_STREAM_MASS + LM_DR_MASS_PLATE_DENSITY, env, dr_step, (uint32_t)dr_reset_key, 0U, cd.p0[0], cd.p1[0], 1.0f);
        X.m_plate = dr_mass(cm, A.seed, LM_DR_STREAM_MASS + LM_DR_MASS_PLATE, env, dr_step, (uint32_t)dr_reset_key, 0U, cm.p0[0], cm.p1[0], X.s_plate * P->plate_mass);
        if (HP) { X.s_plate = held_value(LM_DR_PHYS_ROWS + 1, X.s_plate); X.m_plate = held_value(LM_DR_PHYS_ROWS, X.m_plate); }      // each as stored: a held factor does not re-derive the mass
        if (active && limb == 0) { mrec[env] = X.m_plate; mrec[(size_t)N + env] = X.s_plate; }
      }
    }
    // actuator channels: one kp, one kd and one command latency per env.  The switches are wave-uniform; with the gain channels
    // off the lanes carry the block's kd and kp / kd, with the latency channel off no sub-step looks at the previous command
    {
      const lm_actuator_dr* AD = A.actuator_dr + ((env0 >= A.split) ? 1 : 0);
      const lm_dr_channel& ckp = AD->ch[LM_DR_ACTUATOR_KP]; const lm_dr_channel& ckd = AD->ch[LM_DR_ACTUATOR_KD]; const lm_dr_channel& cl = AD->ch[LM_DR_ACTUATOR_LATENCY];
      float* arec = (float*)(A.actuator_dr + 2);
      X.kd = P->kd; X.gk = P->pd_kp / P->kd; X.lat_on = (VAR >= 1 && cl.enabled) ? 1 : 0; X.lat = 0;
      constexpr int R_ACT = LM_DR_PHYS_ROWS + LM_DR_MASS_ROWS;      // HP: rows of kp, kd, latency
      if (ckp.enabled || ckd.enabled || held(R_ACT) || held(R_ACT + 1)) {
        float kpe = dr_mass(ckp, A.seed, LM_DR_STREAM_ACTUATOR + LM_DR_ACTUATOR_KP, env, dr_step, (uint32_t)dr_reset_key, 0U, ckp.p0[0], ckp.p1[0], P->pd_kp);
        X.kd = dr_mass(ckd, A.seed, LM_DR_STREAM_ACTUATOR + LM_DR_ACTUATOR_KD, env, dr_step, (uint32_t)dr_reset_key, 0U, ckd.p0[0], ckd.p1[0], P->kd);
        if (HP) { kpe = held_value(R_ACT, kpe); X.kd = held_value(R_ACT + 1, X.kd); }
        X.gk = kpe / X.kd;
        if (active && limb == 0) { arec[env] = kpe; arec[(size_t)N + env] = X.kd; }
      }
      if (HP && VAR >= 1 && held(R_ACT + 2)) X.lat_on = 1;
      if (VAR >= 1 && X.lat_on) {
        X.lat = (!HP || cl.enabled) ? dr_latency(cl, A.seed, env, dr_step, (uint32_t)dr_reset_key, (A.nsub < 0) ? P->substeps : A.nsub) : 0;
        if (HP && held(R_ACT + 2)) X.lat = (int)hp[(size_t)(R_ACT + 2) * N + env];      // whole and in [0, substeps]: lm_set_env_params checked it
        if (active && limb == 0) arec[(size_t)2 * N + env] = (float)X.lat;
      }
    }
    if (active) {
      float* ph = A.dr_phys;
#pragma unroll
      for (int c = 0; c < 3; c++) { ph[(size_t)jj[c] * N + env] = X.tmax[c]; ph[(size_t)(12 + jj[c]) * N + env] = X.vmax[c]; ph[(size_t)(30 + jj[c]) * N + env] = X.cj[c]; }
      if (limb == 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) { ph[(size_t)(24 + c) * N + env] = gv[c]; ph[(size_t)(27 + c) * N + env] = fv[c]; }
        ph[(size_t)LM_DR_PHYS_MU * N + env] = X.mu;
      }
    }
  }
#pragma unroll
  for (int a = 0; a < 3; a++) act[a] = clampf(act[a], P->clip_actions);
  // ---- reset_idx (quadruped_pose_control.py:230-299), physical part
  if (do_reset) {
#pragma unroll
    for (int a = 0; a < 3; a++) { q[a] = P->init_q[jj[a]]; qd[a] = 0.f; }
    const float* ip = (MODE == 0) ? P->init_base_pos : P->init_plate_pos; const float* iq = (MODE == 0) ? P->init_base_quat : P->init_plate_quat;
    F.p = v3(ip[0], ip[1], ip[2]); F.q.w = iq[0]; F.q.x = iq[1]; F.q.y = iq[2]; F.q.z = iq[3];
    lin = v3(0, 0, 0); ang = v3(0, 0, 0);
    if (DR) {
      // ---- reset-state channels: a reset that passed the min_frequency gate draws the state it starts from, keyed by the new
      // episode number; the draws and the record stay inside this branch, which a wavefront without a resetting lane skips
      const lm_reset_dr* RD = A.reset_dr + ((env0 >= A.split) ? 1 : 0);
      if (reset_draw) {
        const uint32_t key = (uint32_t)dr_reset_key, e = (uint32_t)env;
        const lm_dr_channel& cq = RD->ch[LM_DR_RESET_JOINT_POS]; const lm_dr_channel& cv = RD->ch[LM_DR_RESET_JOINT_VEL];
        const lm_dr_channel& cp = RD->ch[LM_DR_RESET_POSITION]; const lm_dr_channel& co = RD->ch[LM_DR_RESET_ORIENTATION];
#pragma unroll
        for (int a = 0; a < 3; a++) {
          if (cq.enabled) q[a] = dr_apply(cq.operation, q[a], dr_sample(A.seed, LM_DR_STREAM_RESET + LM_DR_RESET_JOINT_POS, e, key, (uint32_t)jj[a], cq.distribution, cq.p0[0], cq.p1[0]));
          if (cv.enabled) qd[a] = dr_apply(cv.operation, 0.f, dr_sample(A.seed, LM_DR_STREAM_RESET + LM_DR_RESET_JOINT_VEL, e, key, (uint32_t)jj[a], cv.distribution, cv.p0[0], cv.p1[0]));
        }
        if (cp.enabled) {
          float pc[3];
#pragma unroll
          for (int c = 0; c < 3; c++) pc[c] = dr_apply(cp.operation, ip[c], dr_sample(A.seed, LM_DR_STREAM_RESET + LM_DR_RESET_POSITION, e, key, (uint32_t)c, cp.distribution, cp.p0[c], cp.p1[c]));
          F.p = v3(pc[0], pc[1], pc[2]);
        }
        if (co.enabled) {
          float eu[3];
#pragma unroll
          for (int c = 0; c < 3; c++) eu[c] = dr_sample(A.seed, LM_DR_STREAM_RESET + LM_DR_RESET_ORIENTATION, e, key, (uint32_t)c, co.distribution, co.p0[c], co.p1[c]);
          Q4 qe = quat_from_euler(eu[0], eu[1], eu[2]);
          if (co.operation == LM_DR_ADDITIVE) qe = qmul(qe, F.q);      // in the world frame, after the nominal orientation
          const float rn = rsqrtf(qe.w * qe.w + qe.x * qe.x + qe.y * qe.y + qe.z * qe.z);
          F.q.w = qe.w * rn; F.q.x = qe.x * rn; F.q.y = qe.y * rn; F.q.z = qe.z * rn;
        }
      }
      if (active) {      // the state this env starts its episode from (LM_PTR_DR_RESET_STATE), nominal resets included
        float* rs = (float*)(A.reset_dr + 2);
#pragma unroll
        for (int a = 0; a < 3; a++) { rs[(size_t)jj[a] * N + env] = q[a]; rs[(size_t)(12 + jj[a]) * N + env] = qd[a]; }
        if (limb == 0) {
          rs[(size_t)24 * N + env] = F.p.x; rs[(size_t)25 * N + env] = F.p.y; rs[(size_t)26 * N + env] = F.p.z;
          rs[(size_t)27 * N + env] = F.q.w; rs[(size_t)28 * N + env] = F.q.x; rs[(size_t)29 * N + env] = F.q.y; rs[(size_t)30 * N + env] = F.q.z;
        }
      }
    }
  }
  // world -> body-coordinate twist
  {
    M3 R = quat_to_mat(F.q.w, F.q.x, F.q.y, F.q.z);
    F.u = sv(mulT(R, ang), mulT(R, lin));
  }
  M3 Rfix; V3 pfix = v3(P->fixed_base_pos[0], P->fixed_base_pos[1], P->fixed_base_pos[2]);
  Rfix = quat_to_mat(P->fixed_base_quat[0], P->fixed_base_quat[1], P->fixed_base_quat[2], P->fixed_base_quat[3]);
  table_commit(TR, sTab, lane);
  LM_STAMP(0);
  float tau_acc[3] = {0.f, 0.f, 0.f}, tgtq[3] = {0.f, 0.f, 0.f}, qda[3] = {0.f, 0.f, 0.f}; bool qda_set = false;
  constexpr bool pd = (VAR >= 1);
  const int nsub = (A.nsub < 0) ? P->substeps : A.nsub;
  float cf[4] = {0.f, 0.f, 0.f, 0.f};      // CF: contact impulse (world) and loaded sub-steps of this lane's foot
  if (!pd) {
    // ---- take_action (robot.py:452-454): velocity targets
    // velocity mode (every task of the path): the drive's velocity target; effort mode: the torque; position mode (robot.py:448-450):
    // q* = a * act_scale, tau = kp (q* - q) - kd qd = kd (v* - qd) with v* = kp / kd (q* - q), re-evaluated every sub-step
    const float a0[3] = {act[0] * P->act_scale, act[1] * P->act_scale, act[2] * P->act_scale};
    const bool posm = P->drive_mode == LM_DRIVE_POSITION; const float gp = posm ? (DR ? X.gk : P->pd_kp / P->kd) : 0.f;
    for (int s = 0; s < nsub; s++) {
      const float tgt[3] = {posm ? gp * (a0[0] - q[0]) : a0[0], posm ? gp * (a0[1] - q[1]) : a0[1], posm ? gp * (a0[2] - q[2]) : a0[2]};
      substep<MODE, VAR, DR, CF, REG0, HW>(P, sTab, tl, limb, St, F, Rfix, pfix, q, qd, tgt, tau_acc, X, cf);
    }
  } else {
    // ---- custom-controller tasks (quadruped_pose_control_custom_controller.py:255-307): the action integrates the swing / extension
    // position targets; the actuator torque  clamp(kp (q* - q) - kd qd, +-tau_max)  is re-evaluated every sub-step.  It is the same drive
    // as above with damping gain kd and the position-derived velocity target  v* = kp / kd (q* - q)  (implicit in qd, 2-pass clamp).
    float se[3], sep[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      float v = do_reset ? P->init_se[jj[a]] : st[(size_t)(R_SE + jj[a]) * N + env];
      sep[a] = v;
      if (!A.skip_reset || A.nsub != 0) v = fminf(fmaxf(v + act[a] * P->act_scale_se, P->se_lo[jj[a]]), P->se_hi[jj[a]]);
      se[a] = v;
      if (active) st[(size_t)(R_SE + jj[a]) * N + env] = v;
    }
    tgtq[0] = se[0]; tgtq[1] = se[1] + 0.5f * se[2]; tgtq[2] = se[1] - 0.5f * se[2];      // dof1, dof2 = swing + ext/2, dof3 = swing - ext/2
    // command latency (DR): the first X.lat sub-steps still follow the previous command, the targets before this step's action
    const bool lat_on = DR && X.lat_on;
    const float tgtp[3] = {sep[0], sep[1] + 0.5f * sep[2], sep[1] - 0.5f * sep[2]};
    const float g = DR ? X.gk : P->pd_kp / P->kd;
    for (int s = 0; s < nsub; s++) {
      // update_joint_states() runs after every in-task sub-step (…custom_controller.py:296-297): the joint acceleration spans only the
      // trailing acc_substeps (= controlFrequencyInv) sub-steps (robot.py:289-291)
      if (s == nsub - P->acc_substeps) { qda[0] = qd[0]; qda[1] = qd[1]; qda[2] = qd[2]; qda_set = true; }
      const bool prev = lat_on && s < X.lat;
      float tgt[3] = {g * ((prev ? tgtp[0] : tgtq[0]) - q[0]), g * ((prev ? tgtp[1] : tgtq[1]) - q[1]), g * ((prev ? tgtp[2] : tgtq[2]) - q[2])};
      substep<MODE, VAR, DR, CF, REG0, HW>(P, sTab, tl, limb, St, F, Rfix, pfix, q, qd, tgt, tau_acc, X, cf);
    }
  }
  if (CF) store_contact(A.contact, N, env, limb, active, cf, nsub, P->dt);      // nsub = 0 (lm_post_physics): the record is left as it was
  // ---- task-layer state (loaded after the physics: issuing these loads at the top of the last sub-step was measured and gains nothing)
  TaskState S; int episode; float lqd[3];
  if (!(HW == 2 && TS)) { LM_TASK_STATE_LOAD }
  // ---- blow-up guard: the reference only prints NaNs and asserts (quadruped_pose_control.py:550-558); here a non-finite or
  // exploding state is replaced by the reset pose and the env is flagged for reset, so one bad env cannot poison a batch
  int blown = 0;
  {
    float chk = F.p.x + F.p.y + F.p.z + F.q.w + F.q.x + F.q.y + F.q.z + F.u.w.x + F.u.w.y + F.u.w.z + F.u.v.x + F.u.v.y + F.u.v.z
              + q[0] + q[1] + q[2] + qd[0] + qd[1] + qd[2];
    float big = fmaxf(fmaxf(fabsf(qd[0]), fabsf(qd[1])), fmaxf(fabsf(qd[2]), fabsf(F.u.v.x) + fabsf(F.u.v.y) + fabsf(F.u.v.z)));
    blown = quad_sum_i((!(fabsf(chk) < 1.0e30f) || big > 1.0e4f) ? 1 : 0);
    if (blown) {
#pragma unroll
      for (int a = 0; a < 3; a++) { q[a] = P->init_q[jj[a]]; qd[a] = 0.f; }
      const float* ip = (MODE == 0) ? P->init_base_pos : P->init_plate_pos; const float* iq = (MODE == 0) ? P->init_base_quat : P->init_plate_quat;
      F.p = v3(ip[0], ip[1], ip[2]); F.q.w = iq[0]; F.q.x = iq[1]; F.q.y = iq[2]; F.q.z = iq[3];
      F.u = sv(v3(0, 0, 0), v3(0, 0, 0));
      if (active && limb == 0) atomicAdd(reinterpret_cast<unsigned int*>(A.W.stats + 60), 1u);      // contained blow-ups since creation (LM_PTR_STATS)
    }
  }
  LM_STAMP(6);      // task-state loads, reset scatter, blow-up guard
#if defined(LM_HELPER_WAVE) && LM_HELPER_WAVE >= 2
  // k_step_h3's tail (TS): behind barrier R1 the task-layer state is in TASK_SLOT, where wavefront 1 put it while this wavefront ran the second
  // half of the last sub-step; wavefront 1 ends behind R1
  if (HW == 2 && TS) {
    hw_barrier();
    const float4 t0 = St.get(TASK_SLOT), t1 = St.get(TASK_SLOT + 1), t2 = St.get(TASK_SLOT + 2), t3 = St.get(TASK_SLOT + 3), t4 = St.get(TASK_SLOT + 4);
    S.succ = __float_as_int(t0.x); S.consec = __float_as_int(t0.y); S.greset = __float_as_int(t0.z); S.reset = __float_as_int(t0.w);
    S.progress = __float_as_int(t1.x); episode = __float_as_int(t1.y); S.lact[0] = t1.z; S.lact[1] = t1.w;
    S.lact[2] = t2.x; lqd[0] = t2.y; lqd[1] = t2.z; lqd[2] = t2.w;
    S.ltip = v3(t3.x, t3.y, t3.z); S.goal.w = t3.w; S.goal.x = t4.x; S.goal.y = t4.y; S.goal.z = t4.z;
    S.lrd = 0.f; S.ltgt[0] = S.ltgt[1] = S.ltgt[2] = 0.f;
  }
#endif
  // ---- read-back (robot.py:276-321)
  TaskIn I;
  M3 Rf = quat_to_mat(F.q.w, F.q.x, F.q.y, F.q.z);
  I.fp = F.p; I.fq = F.q; I.lin = mul(Rf, F.u.v); I.ang = mul(Rf, F.u.w);
  {
    LimbKin K; float z3[3] = {0.f, 0.f, 0.f};
    limb_kinematics(tl, q, z3, K);
    V3 x, k2, k3; limb_points(tl, K, x, k2, k3);
    M3 Rb = (MODE == 0) ? Rf : Rfix; V3 pb = (MODE == 0) ? F.p : pfix;
    I.tipw = pb + mul(Rb, x); I.knee2 = pb + mul(Rb, k2); I.knee3 = pb + mul(Rb, k3);
  }
  const float acc_dt_inv = P->acc_dt_inv, ctrl_dt_inv = P->ctrl_dt_inv, torque_div = pd ? P->torque_div : 1.f;      // one batch of loads (see task_eval)
#pragma unroll
  for (int a = 0; a < 3; a++) { I.q[a] = q[a]; I.qd[a] = qd[a]; I.acc[a] = (pd && qda_set) ? (qd[a] - qda[a]) * acc_dt_inv : (qd[a] - lqd[a]) * ctrl_dt_inv; I.act[a] = act[a];
    I.torque[a] = pd ? tau_acc[a] / torque_div : 0.f; I.tgtq[a] = tgtq[a]; }      // logged torque = sum over sub-steps / control_decimal (:307)
  TaskOut O;
  task_eval<MODE, VAR>(P, limb, envl, I, S, O, sObs, sSt);
  LM_STAMP(7);      // read-back kinematics + task layer
  if (blown) S.reset = 1;
  // ---- store state
  if (active) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      st[(size_t)(R_Q + jj[a]) * N + env] = q[a]; st[(size_t)(R_QD + jj[a]) * N + env] = qd[a];
      st[(size_t)(R_LACT + jj[a]) * N + env] = S.lact[a]; st[(size_t)(R_LQD + jj[a]) * N + env] = qd[a];
    }
    st[(size_t)(R_LTIP + 3 * limb) * N + env] = S.ltip.x; st[(size_t)(R_LTIP + 3 * limb + 1) * N + env] = S.ltip.y; st[(size_t)(R_LTIP + 3 * limb + 2) * N + env] = S.ltip.z;
    if (pd) {
#pragma unroll
      for (int a = 0; a < 3; a++) st[(size_t)(R_LTGT + jj[a]) * N + env] = S.ltgt[a];
      if (limb == 0) st[(size_t)R_LRD * N + env] = S.lrd;
    }
    if (limb == 0) {
      st[(size_t)(fb + 0) * N + env] = F.p.x; st[(size_t)(fb + 1) * N + env] = F.p.y; st[(size_t)(fb + 2) * N + env] = F.p.z;
      st[(size_t)(fb + 3) * N + env] = F.q.w; st[(size_t)(fb + 4) * N + env] = F.q.x; st[(size_t)(fb + 5) * N + env] = F.q.y; st[(size_t)(fb + 6) * N + env] = F.q.z;
      st[(size_t)(fb + 7) * N + env] = I.lin.x; st[(size_t)(fb + 8) * N + env] = I.lin.y; st[(size_t)(fb + 9) * N + env] = I.lin.z;
      st[(size_t)(fb + 10) * N + env] = I.ang.x; st[(size_t)(fb + 11) * N + env] = I.ang.y; st[(size_t)(fb + 12) * N + env] = I.ang.z;
      st[(size_t)(R_GOAL + 0) * N + env] = S.goal.w; st[(size_t)(R_GOAL + 1) * N + env] = S.goal.x; st[(size_t)(R_GOAL + 2) * N + env] = S.goal.y; st[(size_t)(R_GOAL + 3) * N + env] = S.goal.z;
    }
  }
  DrOut DO; DO.drc = A.drc; DO.seed = A.seed; DO.dr_step = dr_step; DO.rand_buf = dr_rand_buf; DO.reset_key = dr_reset_key;
#ifdef LM_WAVES2
  DO.sKey = reinterpret_cast<uint32_t*>(sSt + ENVS_PER_WAVE * 93);      // behind the output staging, which lives in the stash's memory in this build
#else
  DO.sKey = reinterpret_cast<uint32_t*>(sStash);      // the stash is dead after the last sub-step
#endif
  LM_STAMP(8);      // state stores issued
  write_outputs<DR, DEFER, (VAR == 1) ? LM_MAX_OBS : 64, OW>(P, A.W, N, env0, lane, limb, env, active, S, O, cnt, episode, sObs, sSt, DO);
  LM_STAMP(10);     // the reduction's round trips
}

#if defined(LM_HELPER_WAVE) && LM_HELPER_WAVE >= 2
// The tail of k_step_h3's wavefront 1 (LM_H3_TAIL_STATE).  Behind its last sub-step barrier (with no sub-step: at once) it fetches
// the task-layer state of lane l of wavefront 0, by the lines every step kernel runs (LM_TASK_STATE_LOAD), into TASK_SLOT, passes barrier R1 and
// ends.  It reads what wavefront 0 reads, and wavefront 0 writes none of it before R1: cnt and the task rows of the state are stored behind the
// task layer.  Counters travel as their bit patterns.  Same bits as k_step: plain copies of memory, and in a resetting lane the goal quaternion,
// a complete result of quat_from_euler that k_step holds rounded too and only uses as an operand.  R1 stands in straight-line code in all three
// wavefronts (the terms helper passes it in front of its output barrier); with the switch off it is compiled in none
LM_DEV void helper_task_state(const StepArgs& A, const lm_params* __restrict__ P, float4* sStash, int lane) {
  const int limb = lane & 3, envl = lane >> 2;
  const int env0 = lm_block() * ENVS_PER_WAVE, envr = env0 + envl, N = A.N;
  const int env = (envr < N) ? envr : (N - 1);
  const int jj[3] = {limb, 4 + 2 * limb, 5 + 2 * limb};
  const bool do_reset = (A.cnt[3 * (size_t)N + env] != 0) && !A.skip_reset;
  TaskState S; int episode; float lqd[3];
  task_state_load<0, 0>(A, P, A.state, A.cnt, N, env, limb, jj, do_reset, S, episode, lqd);
  Stash St; St.base = sStash; St.lane = lane;
  St.put(TASK_SLOT, __int_as_float(S.succ), __int_as_float(S.consec), __int_as_float(S.greset), __int_as_float(S.reset));
  St.put(TASK_SLOT + 1, __int_as_float(S.progress), __int_as_float(episode), S.lact[0], S.lact[1]);
  St.put(TASK_SLOT + 2, S.lact[2], lqd[0], lqd[1], lqd[2]);
  St.put(TASK_SLOT + 3, S.ltip.x, S.ltip.y, S.ltip.z, S.goal.w); St.put(TASK_SLOT + 4, S.goal.x, S.goal.y, S.goal.z, 0.f);
  hw_barrier();      // R1
}
#endif

// The step kernels.  One launch per step(); a wavefront picks its specialisation (task mode x actuator family) from the kernel arguments.  The
// velocity-drive tasks (k_step: the headline) and the PD-actuator families (k_step_pd) are separate kernels, so that the register allocation
// and code layout of the one do not move when the other is edited; both blocks of a co-training engine are of one actuator family (lm_create).
#ifdef LM_STAMPS
#define LM_STEP_PROLOGUE \
  if (threadIdx.x < 64) lm_stamp_lds[threadIdx.x] = 0; \
  __builtin_amdgcn_s_waitcnt(0xc07f); __builtin_amdgcn_s_barrier(); \
  { unsigned long long t0_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0_) :: "memory"); if ((threadIdx.x & 63) == 0) lm_stamp_lds[16 * (threadIdx.x >> 6) + 15] = t0_; } \
  LM_STAMP(11); LM_STAMP(12);      /* two stamps back to back: bucket 12 = the cost of a stamp */ \
  const unsigned long long rt0_ = __builtin_amdgcn_s_memrealtime(), mt0_ = __builtin_amdgcn_s_memtime();
#define LM_STEP_EPILOGUE \
  { const unsigned long long rt1_ = __builtin_amdgcn_s_memrealtime(), mt1_ = __builtin_amdgcn_s_memtime(); \
    if (threadIdx.x == 0) { lm_stamp_lds[13] = mt1_ - mt0_; lm_stamp_lds[14] = rt1_ - rt0_; } } \
  __builtin_amdgcn_s_waitcnt(0xc07f); \
  if (threadIdx.x < 64 && blockIdx.x < 1024) lm_stamp_out[blockIdx.x * 64 + threadIdx.x] = lm_stamp_lds[threadIdx.x];
#else
#define LM_STEP_PROLOGUE
#define LM_STEP_EPILOGUE
#endif
#ifdef LM_WAVES2
#define LM_STEP_SMEM(NOBS) \
  __shared__ __attribute__((aligned(16))) float sTab[LM_ITAB_FLOATS + 2]; \
  __shared__ float4 sStash[STASH_SLOTS * 64]; \
  static_assert(ENVS_PER_WAVE * ((NOBS) + 93 + 3) * 4 <= STASH_SLOTS * 64 * 16, "output staging must fit in the stash"); \
  float* sObs = reinterpret_cast<float*>(sStash); float* sSt = sObs + ENVS_PER_WAVE * (NOBS); \
  const int env0 = lm_block() * ENVS_PER_WAVE; \
  const lm_params* P = A.params + ((env0 >= A.split) ? 1 : 0); \
  const int kind = A.kind[(env0 >= A.split) ? 1 : 0];
#else
#define LM_STEP_SMEM(NOBS) \
  __shared__ __attribute__((aligned(16))) float sTab[LM_ITAB_FLOATS + 2]; \
  __shared__ __attribute__((aligned(16))) float sObs[ENVS_PER_WAVE * (NOBS)]; \
  __shared__ __attribute__((aligned(16))) float sSt[ENVS_PER_WAVE * 93]; \
  __shared__ float4 sStash[STASH_SLOTS * 64]; \
  const int env0 = lm_block() * ENVS_PER_WAVE; \
  const lm_params* P = A.params + ((env0 >= A.split) ? 1 : 0); \
  const int kind = A.kind[(env0 >= A.split) ? 1 : 0];
#endif
