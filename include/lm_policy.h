/*
 * lm_policy.h -- C ABI of the policy forward passes (GNN, MLP), the action sampling and the fused rollout (part of liblm_engine.so).
 *
 * Replaces, for inference, the torch modules of RobotLearning/omniisaacgymenvs/scripts/graph_model_orebot_ov.py
 * (GraphNet :82-110, GraphLayer :11-80, Action_Layer :215-226, Value_Layer :228-241) as instantiated by
 * scripts/skrl_ppo_locomanipulation_vertical.py:44-49 (hidden_features = out_features = 32).
 */
#ifndef LM_POLICY_H
#define LM_POLICY_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Number of floats in the packed parameter block:
 *   input_layer1.weight (32,16) .bias (32) | input_layer2.weight (32,4) .bias (32) |
 *   3 x { linear1.weight (32,64) .bias (32) | linear2.weight (32,32) .bias (32) } |
 *   action_layer.weight (32) .bias (1) | value action_layer.weight (32) .bias (1)          (all row-major, torch layout) |
 *   observation preprocessor: mean (64) | 1/(sqrt(var)+eps) (64) | clip (1)   (identity: 0, 1, +inf) */
int lm_gnn_param_count(void);

/* obs: device float [batch][64] (the env's observation layout, quadruped_pose_control.py:358-371);
 * params: device float [lm_gnn_param_count()]; mean: device float [batch][12] (node order = dof1 a1..a4, dof2 a1..a4,
 * dof3 a1..a4); value: device float [batch].  Returns 0, -1 (bad argument) or -2 (launch failure).
 * obs and params must be 16-byte aligned (both are read with 16-byte loads): -1 otherwise, nothing is launched. */
int lm_gnn_forward(const float* obs, int batch, const float* params, float* mean, float* value, void* stream);

/* MLP policy of the locomotion / manipulation scripts (scripts/skrl_ppo_locomotion.py:30-40: shared trunk
 * Linear(64,256) ELU Linear(256,128) ELU Linear(128,64) ELU, mean_layer Linear(64,12), value_layer Linear(64,1)) with the
 * observation preprocessor (skrl RunningStandardScaler, :96-99) folded in.  `params` is the block produced by
 * locomanipulationrl_amd.policies.mlp_model.pack_mlp_params: biases and the scaler as floats; every weight matrix as 32-bit words
 * [out/16][K-blocks of 32][64 lanes][8] in the operand order of v_mfma_f32_16x16x32_f16, each weight split into two fp16 halves
 * (w = hi + lo; words 0..3 the hi halves, 4..7 the lo halves) - the tile computes fp32 products as four half products, fp32-level accuracy
 * (layout and column map: csrc/lm_policy_dev.h; round 4 - rounds 1-3 packed plain floats in v_mfma_f32_16x16x4_f32 order, same word counts for
 * num_obs 64).  lm_mlp_param_count() is its length.  Outputs as lm_gnn_forward (mean in the env's action order). */
int lm_mlp_param_count(void);
int lm_mlp_forward(const float* obs, int batch, const float* params, float* mean, float* value, void* stream);
/* The same network on the 88-wide observation of the custom-controller tasks (…custom_controller.py:432-455) or the 64-wide one:
 * num_obs in {64, 88}; the packed block is  mean num_obs | 1/std num_obs | clip (+3 pad) | W1q 256 x (num_obs padded to a multiple of 32) | ... as above.
 * obs and params must be 16-byte aligned, as for lm_gnn_forward: -1 otherwise (and for another num_obs), nothing is launched. */
int lm_mlp_param_count_obs(int num_obs);
int lm_mlp_forward_obs(const float* obs, int batch, int num_obs, const float* params, float* mean, float* value, void* stream);

/* ---- fused rollout: policy forward -> gaussian action sampling -> lm_step, T times, as ONE hipGraph launch.
 * Replaces the per-step Python of the reference's trainer loop (skrl SequentialTrainer / scripts/random_policy.py:52-61:
 * agent.act -> env.step -> agent.record_transition) for the duration of a rollout, during which the policy is constant. */
struct lm_engine;
typedef struct lm_rollout lm_rollout;
enum { LM_POLICY_MLP = 0, LM_POLICY_GNN = 1 };

/* Gaussian policy sampling (skrl GaussianMixin.act): actions = mean + exp(log_std) * eps, logp = sum_j log N(actions_j; mean_j, std_j).
 * eps is a counter-based normal keyed by (seed, env, episode_count, progress_buf) read from the engine's counters
 * (cnt = lm_ptr(h, LM_PTR_CNT)), so no generator state is kept and no step repeats a draw.
 *   mean device [n_envs][12], log_std device [12], actions device [n_envs][12] (not clamped: lm_step clamps), logp device [n_envs] */
int lm_sample_actions(const float* mean, const float* log_std, const int64_t* cnt, int n_envs, uint32_t seed,
                      float* actions, float* logp, void* stream);

/* Plan a rollout of T steps on `env`.  All buffers are device memory owned by the caller and must stay valid:
 *   obs [T+1][N][lm_num_obs(env)]   obs[0] = the current (clipped) observations on entry; obs[t+1] = those returned by step t
 *                      (88-wide observations: MLP policy only)
 *   actions [T][N][12], logp [T][N], values [T+1][N] (value head output; values[T] bootstraps), rewards [T][N], dones int64 [T][N],
 *   extras [T][LM_NUM_EXTRAS] (may be NULL)
 *   policy_params / log_std: device blocks read at run time (update them in place between runs)
 * policy_params and obs must be 16-byte aligned (16-byte loads, both policies): LM_EINVAL (-1) otherwise, no plan is made. */
int lm_rollout_create(lm_rollout** out, struct lm_engine* env, int policy, const float* policy_params, const float* log_std, int T,
                      uint32_t noise_seed, float* obs, float* actions, float* logp, float* values, float* rewards, int64_t* dones,
                      float* extras);
/* Enqueue the rollout on `stream`.  use_graph: LM_ROLLOUT_ENQUEUE enqueues the 2T+1 kernels, LM_ROLLOUT_GRAPH replays a hipGraph of them
 * captured on first use (one launch), LM_ROLLOUT_PERSISTENT runs the whole rollout inside ONE kernel (every block keeps its 16 envs for
 * the T steps, the observations go from the step to the next forward through LDS; un-randomised engines only, -1 otherwise).
 * A persistent block occupies a whole compute unit, so the mode pays up to 16 x (compute units) envs = 4096 on MI355X and serialises beyond;
 * LM_ROLLOUT_AUTO picks it within that size on engines that support it and the graph otherwise.
 * All modes write bit-identical buffers. */
#define LM_ROLLOUT_ENQUEUE 0
#define LM_ROLLOUT_GRAPH 1
#define LM_ROLLOUT_PERSISTENT 2
#define LM_ROLLOUT_AUTO 3
int lm_rollout_run(lm_rollout* r, int use_graph, void* stream);
int lm_rollout_destroy(lm_rollout* r);

/* ---- evaluation: mean actions and episode records (what the reference's scripts do with eval = True: agent.set_mode('eval') and the
 * trainer's evaluation loop).  Both are switches of a plan, off after lm_rollout_create; a plan that uses neither runs the kernels and
 * writes the bits it did before they existed.  Flipping one invalidates a captured graph as lm_set_seed does (re-captured on the next
 * run, never refused).  All three return 0 or LM_EINVAL (-1): a null plan / handle, a calling thread whose current device is not the
 * engine's, and lm_episode_update with a null rewards, dones or record.
 *
 * Deterministic mode (on != 0): actions[t] = the forward's mean, bit for bit (the mean itself, not mean + exp(log_std) * 0, so an
 * overflowing exp(log_std) cannot make a NaN); logp[t] = the stochastic expression at eps = 0, sum_j (-log_std_j - ln sqrt(2 pi)) in the
 * same summation order (groups of four, then (p0 + p1) + (p2 + 0)); no normal is drawn and noise_seed is not read.  Values, observations,
 * rewards, dones and extras are written as always.  lm_sample_actions belongs to no plan and always samples. */
int lm_rollout_set_deterministic(lm_rollout* r, int on);

/* Episode record: a caller-owned device buffer float [LM_EPISODE_ROWS][N] that the caller zeroes to start a measurement and that persists
 * across runs (episodes cross rollout boundaries).  Rows, per env:
 *   0 running return | 1 running length | 2 episodes completed | 3 sum of the returns of completed episodes | 4 sum of their lengths |
 *   5 ended by goal | 6 ended by timeout | 7 ended by failure | 8 return of the last completed episode
 * After step t of env e, with r = rewards[t][e], d = dones[t][e], g = the env's goal_reset_buf after that step and M = max_episode of
 * the env's parameter block (the two blocks of a co-training engine may differ):
 *   if (cap > 0 && row2 >= cap) skip the env;          the first `cap` episodes of EVERY env: no bias towards short episodes
 *   row0 = row0 + r;  row1 = row1 + 1;                 plain fp32 adds, in step order
 *   if (d) { row2 += 1; row3 = row3 + row0; row4 = row4 + row1;  g ? row5 += 1 : (row1 >= M - 1 ? row6 += 1 : row7 += 1);
 *            row8 = row0; row0 = 0; row1 = 0; }
 * A length counts the step that resets the env, as progress_buf does: zero the record when every env is about to reset (lm_reset_all), or
 * the first episode of an env is seen shorter than it was and its timeout is counted as a failure.
 * The reward of a step belongs to the episode that step ends (the env is reset at the start of the next step).  A failure on the very step
 * the timeout would fire counts as a timeout.  The outcome is read from the flags, never from the reward (fall_pen is 0.0 in the shipped
 * tasks).  Counts and lengths are floats: exact below 2^24.  record == NULL switches recording off; episode_cap <= 0 means no cap.
 * Enqueue, graph and persistent runs fill identical buffers and identical records.  The persistent kernels with either switch on are builds
 * of their own.  A recording build is shipped only where it compiles with 0 bytes of scratch memory: the MLP on 64-wide observations.  For
 * the MLP on 88-wide observations and for the GNN, LM_ROLLOUT_PERSISTENT returns -1 for a plan with a record attached and LM_ROLLOUT_AUTO
 * takes the graph; deterministic mode alone runs persistent for every policy.  Randomised engines and engines with contact reporting on
 * keep their rule (graph / enqueue only). */
#define LM_EPISODE_ROWS 9
int lm_rollout_set_episode_record(lm_rollout* r, float* record, int episode_cap);

/* The same update as one small launch, for callers that step with lm_step themselves: rewards [N] and dones int64 [N] as lm_step wrote
 * them for the step that has just been enqueued on `stream`; g and M are read from the engine.  The enqueue and graph rollouts call it
 * after each lm_step. */
int lm_episode_update(struct lm_engine* h, const float* rewards, const int64_t* dones, float* record, int episode_cap, void* stream);

/* ---- trajectory record: what K chosen envs did, one row per control step (what the reference's co-training task does with RECORD_JOINT = True,
 * tasks/joint_train_locomanipulation/joint_locomanipulation.py:36-46, 556-563, 861-874: it appends the 12 driven joint positions of one env
 * after every control step until that env's reset flag is raised, then np.save()s them).  Like the episode record it is a switch of a plan,
 * off after lm_rollout_create; a plan or engine that does not use it launches the kernels and writes the bits it did before it existed.
 *
 * Two caller-owned device buffers, which persist across runs (episodes cross rollout boundaries) and which the caller zeroes to start a
 * measurement; K = 1 .. LM_TRAJ_MAX_ENVS tracked env ids, distinct, in [0, N):
 *   rows   float [K][max_rows][LM_TRAJ_COLS]   slot-major: one slot's trajectory is a contiguous slice; a row is 256 B; 16-byte aligned
 *   header int32 [K][4]                        per slot { rows written, episodes completed, rows dropped, 0 }
 * After step t, a row of slot k tracking env e is a column-by-column COPY of what stands in the engine's state (the SoA rows R_* of
 * csrc/lm_dynamics.h, lm_ptr LM_PTR_STATE), in its counters (LM_PTR_CNT) and in the step's outputs after that step - no arithmetic, so every
 * path writes the same bits:
 *   columns  0-11  q (R_Q), in the order robot.joint_positions exposes: the order of the reference's recordings
 *           12-23  qd (R_QD)
 *           24-30  free body position and quaternion (w, x, y, z): R_FB0 + 0..6, the base, for an env of a locomotion block; R_FB1 + 0..6, the
 *                  plate, for an env of a manipulation block (a co-training engine: chosen per env by split_env)
 *           31-42  R_LACT: the clamped actions the step applied
 *           43-54  R_LTIP (below)
 *           55-58  R_GOAL: the goal quaternion (w, x, y, z)
 *           59     rewards[t][e]
 *           60     dones[t][e] != 0, as 0.0 / 1.0
 *           61     goal_reset_buf (LM_PTR_CNT row 2) != 0, as 0.0 / 1.0
 *           62     progress_buf (row 4) as float
 *           63     episode_count (row 5) as float
 * R_LTIP after a step holds the four foot-tip positions (limb-major x, y, z) of the POST-step state in the frame of the robot's base body -
 * the moving base for a locomotion env, the fixed inverted base for a manipulation env: the task layer's `btip`, which it keeps as the
 * next step's last_tip.  They are NOT world positions (lm_forward_kinematics gives those); for an env reset by this step they are the tips
 * of the reset pose after its first control step.
 * An env flagged done still shows its TERMINAL state in that row: the reset happens at the start of the next lm_step.
 *
 * Update rule, per slot after each step (hdr = the slot's header, cap = episode_cap, <= 0: no cap):
 *   if (cap > 0 && hdr.episodes >= cap) skip;
 *   if (hdr.rows < max_rows) { write row hdr.rows; hdr.rows += 1; } else hdr.dropped += 1;      never a store past the slot
 *   if (done) hdr.episodes += 1;
 * With cap = 1, a record zeroed when every env is about to reset (lm_reset_all) is exactly the reference's recording: one row per control
 * step from the reset step up to and including the terminal step.
 *
 * lm_rollout_set_trajectory_record validates on the host - LM_EINVAL for a null plan, K outside [1, LM_TRAJ_MAX_ENVS], an id outside [0, N)
 * or repeated, null rows / header, max_rows < 1, rows not 16-byte aligned, a calling thread whose current device is not the engine's - and
 * copies the ids into device memory owned by the plan (-2 if that allocation or copy fails).  It is SYNCHRONOUS (a blocking host-to-device copy, as the randomisation setters of
 * lm_engine.h): do not call it while a run of the plan is in flight.  env_ids_host == NULL or K == 0 switches recording off.  Flipping it
 * invalidates a captured graph as lm_rollout_set_episode_record does (re-captured on the next run, never refused).
 * Enqueue and graph runs update the record after every lm_step (after lm_episode_update when both are attached); enqueue, graph and
 * persistent runs fill identical buffers and identical records.  The persistent kernels that keep a trajectory record are builds of their
 * own, shipped - the rule of the episode record - only where they compile with 0 bytes of scratch memory: the MLP on 64-wide observations,
 * alone and together with deterministic mode and / or an episode record.  For the MLP on 88-wide observations and for the GNN,
 * LM_ROLLOUT_PERSISTENT returns -1 for a plan with a trajectory record attached and LM_ROLLOUT_AUTO takes the graph; randomised engines and
 * engines with contact reporting on keep their rule (graph / enqueue only). */
#define LM_TRAJ_COLS 64
#define LM_TRAJ_MAX_ENVS 256
int lm_rollout_set_trajectory_record(lm_rollout* r, const int32_t* env_ids_host, int K, float* rows, int32_t* header, int max_rows,
                                     int episode_cap);

/* The same update as one small launch (one wavefront per slot, lane = column), for callers that step with lm_step themselves: env_ids_dev
 * device int32 [K]; rewards [N] and dones int64 [N] as lm_step wrote them for the step that has just been enqueued on `stream`.  An id
 * outside [0, N) is skipped by the kernel, not read through.  Any engine family: PD, randomised, contact reporting, co-training.
 * Returns 0, LM_EINVAL (a null argument, K outside [1, LM_TRAJ_MAX_ENVS], max_rows < 1, misaligned rows, the wrong device) or -2. */
int lm_trajectory_update(struct lm_engine* h, const int32_t* env_ids_dev, int K, const float* rewards, const int64_t* dones, float* rows,
                         int32_t* header, int max_rows, int episode_cap, void* stream);

/* ---- replay of recorded joint motions (csrc/lm_replay.hip): N envs are driven along R recorded joint trajectories (the format of the
 * reference's RECORD_JOINT files and of the trajectory record's q columns) and every env is scored against its recording where the data lives.
 * With per-env parameters held (lm_set_env_params) one run scores a whole grid of physics parameters: a parameter fit, or system
 * identification from joint logs.  No step kernel, launch path or record layout changes: the caller steps with lm_step and calls
 * lm_replay_update after every step, as lm_episode_update / lm_trajectory_update are used.
 *
 * A replay plan belongs to an engine and owns device copies of
 *   rec float [R][T_max][12]   the joint rows to score against, in the order of robot.joint_positions (state rows R_Q + 0..11)
 *   act float [R][T_max][12]   the open-loop action applied at step s (row 0: the reset step, conventionally zero)
 *   len int32 [R]              rows of each recording, window_rows <= len <= T_max
 *   env_rec int32 [N]          which recording env e replays; -1: the env takes no part (zero actions, its record column is never written)
 * lm_replay_create is SYNCHRONOUS (blocking copies, like lm_rollout_set_trajectory_record).  servo != 0 replaces the action table by a
 * proportional steer back onto the recording (below); hold in [0, 8] further zero-action rows are scored after a recording's last row
 * (returns and termination only) so that a success streak that started late can complete; inv_full = 1 / (act_scale x control period), the
 * reciprocal of the joint displacement of a saturated action, computed by the caller (the product build divides to 1 ulp);
 * v2_thresh = sin^2(thresh / 2) for the success window thresh of the task (rot_dist = 2 asin |v| <= thresh  <=>  |v|^2 <= v2_thresh);
 * track_tol the joint-step error below which a joint-step counts as tracked.
 * LM_EINVAL (-1, reason in lm_last_error; nothing is allocated) for: a null argument; R < 1; T_max < 1; a length outside [window_rows, T_max]
 * (window_rows < 1 included); an id outside [-1, R); hold outside [0, 8]; a table entry, inv_full, v2_thresh or track_tol that is not finite;
 * a calling thread whose current device is not the engine's; an engine with a block that is not variant 0 in LM_DRIVE_VELOCITY with 64-wide
 * observations (PD targets are not joint-rate actions).  -2 if an allocation or copy fails.
 *
 * lm_replay_update is called after lm_step number s (s = 0 is the reset step: call it on an engine whose envs are all about to reset), on the
 * stream the step was enqueued on: ONE launch, one thread per env, SoA accesses, no atomics.  It reads LM_PTR_STATE rows R_Q + 0..11,
 * LM_PTR_CNT rows 2 (goal_reset_buf) and 3 (reset_buf), obs [N][64] and rewards [N] as that step wrote them (obs columns 7..9, the vector
 * part of the orientation error, are far below any clip), and writes
 *   record float [LM_REPLAY_ROWS][N]   caller-owned; before step 0: rows 2 and 9 = -1, row 11 = +inf, everything else 0
 *   actions_next float [N][12]         the actions of step s + 1 (may be the buffer step s read)
 * Rule per env with r = env_rec[e] >= 0 and T = len[r]; fp32, in the order written, no contraction:
 *   if (finished || s >= T + hold) { actions_next = 0; return; }
 *   q_j = state[R_Q + j][e];  v2 = (o7*o7 + o8*o8) + o9*o9  (obs[e][7..9]);  rew = rewards[e]
 *   if (s < T) {
 *     d_j = q_j - rec[r][s][j];  m = max_j |d_j|
 *     if (s == 0) { row0_err = m; v2_first = v2; }
 *     qerr = max(qerr, m);  abs_sum += sum_j |d_j|;  sq_sum += sum_j d_j^2
 *     if (s >= 1) { e_j = (q_j - qprev_j) - (rec[r][s][j] - rec[r][s-1][j]);  tracked += #{ |e_j| < track_tol };  if (s <= 4) early += sum_j |e_j|; }
 *     if (v2 <= v2_thresh) { if (first_succ < 0) first_succ = s;  if (s >= T - window_rows) in_window += 1; }
 *     min_v2 = min(min_v2, v2);  if (s >= T - window_rows) window_return += rew;
 *     rows += 1;  qprev = q;
 *   }
 *   ret += rew;
 *   if (cnt[3][e] != 0) { finished = 1; done_at = s; goal_at_done = (cnt[2][e] != 0); }
 *   actions_next_j = (finished || s + 1 >= T) ? 0 : servo ? clamp((rec[r][s+1][j] - q_j) * inv_full, -1, 1) : act[r][s+1][j]
 * (the sums over j run j = 0 .. 11 from zero and are then added to the running value).  An env with r = -1 gets actions_next = 0.
 * Record rows:  0 rows | 1 finished | 2 done_at | 3 goal_at_done | 4 row0_err | 5 qerr | 6 sq_sum | 7 tracked | 8 early | 9 first_succ |
 *   10 in_window | 11 min_v2 | 12 ret | 13 window_return | 14 v2_first | 15 abs_sum | 16-27 qprev | 28 saturated | 29 cmd_err (both: PD plans in
 *   targets mode only, below; otherwise never written) | 30-31 never written.
 * Counts and rows are floats: exact below 2^24.  The rule restates the host replay the project's evidence was produced with: rows up to and
 * including the terminal row, statistics over recorded rows only, `hold` zero-action rows after the recording; one difference: a reset flag
 * raised on row 0 ends the replay.
 * lm_replay_update returns LM_EINVAL for a null argument, s < 0, actions_next that is not 16-byte aligned (an env's 12 actions leave as three
 * 16-byte stores) or a foreign device - nothing is launched; -2 for a launch failure.  lm_replay_steps: the number of
 * steps a run takes, max over the recordings in use of len + hold (0 when no env takes part; LM_EINVAL for a null plan).
 *
 * PD-actuator engines: lm_replay_create_pd makes a plan of the same type for an engine whose every block is variant 1 (custom controller,
 * 88-wide observations), variant 2 (position control) or variant 0 in LM_DRIVE_POSITION; co-training engines with two such blocks are
 * accepted and an env's block is chosen by the engine's split_env.  What such a robot logs is a command log plus measured joints:
 *   rec float [R][T_max][12]   the joint rows to score against, as above
 *   cmd float [R][T_max][12]   LM_REPLAY_CMD_ACTIONS: cmd[r][s] = the action applied at step s (row 0: the reset step's; the trajectory
 *                              record's last_actions columns are these);  LM_REPLAY_CMD_TARGETS: cmd[r][s] = the 12 joint position targets
 *                              commanded for step s, in the joint order of rec
 * len, env_rec, hold, window_rows, v2_thresh and track_tol as above.  The plan reads variant, act_scale_se, act_scale and num_obs from the
 * engine's own blocks; the caller passes no scale.  The reciprocals inv_act_scale_se = 1 / act_scale_se (variants 1 / 2) and
 * inv_act_scale = 1 / act_scale (variant 0) are formed once on the host, in float.  LM_EINVAL (reason in lm_last_error; nothing is
 * allocated) for everything lm_replay_create refuses except the engine family, and for a block in velocity or effort drive, a cmd_mode
 * outside {0, 1} and a cmd entry that is not finite.  lm_replay_steps and lm_replay_destroy serve both kinds of plan.
 * lm_replay_update on a PD plan takes obs [N][lm_num_obs(engine)] (columns 7..9 are the orientation-error vector in all three layouts) and
 * launches k_replay_update_pd: one thread per env, SoA accesses, no atomics, no LDS, no contraction.  The scoring rule above stays word for
 * word (rows 0..27, finished, hold, the window).  The last line of the rule becomes, with se_j = state[R_SE + j][e] as step s left it:
 *   actions mode:  actions_next_j = (finished || s + 1 >= T) ? 0 : cmd[r][s+1][j]
 *   targets mode, for a not-finished env with s + 1 < T (otherwise actions_next = 0), t = cmd[r][s+1]:
 *     variants 1 / 2:  for limb l = 0 .. 3 (rows l: dof1, 4+2l: swing, 5+2l: extension - the indices the step uses for R_Q and R_SE)
 *                        c[l] = t[l];  c[4+2l] = 0.5f * (t[4+2l] + t[5+2l]);  c[5+2l] = t[4+2l] - t[5+2l];      (the inverse of the step's targets)
 *                      raw_j = (c_j - se_j) * inv_act_scale_se
 *     variant 0 in LM_DRIVE_POSITION:  raw_j = t_j * inv_act_scale
 *     actions_next_j = clamp(raw_j, -1, 1);  saturated += #{ j : |raw_j| > 1 }
 *   targets mode, variants 1 / 2, 1 <= s < T (inside the `if (s < T)` block), c formed from t = cmd[r][s] as above:
 *     cmd_err = max(cmd_err, max_j |c_j - se_j|)      the command the engine holds after step s against the command logged for it
 * A saturated count or a cmd_err above rounding says that the log cannot be reproduced through this task's rate-limited (act_scale_se per
 * step), range-limited (se_lo .. se_hi) action interface.  In actions mode and on velocity plans rows 28 and 29 are never written. */
#define LM_REPLAY_ROWS 32
#define LM_REPLAY_CMD_ACTIONS 0   /* cmd[r][s] = the action applied at step s (row 0: the reset step's) */
#define LM_REPLAY_CMD_TARGETS 1   /* cmd[r][s] = the 12 joint position targets commanded for step s, joint order of rec */
typedef struct lm_replay lm_replay;
int lm_replay_create(lm_replay** out, struct lm_engine* h, const float* rec_host, const float* act_host, const int32_t* len_host, int R, int T_max,
                     const int32_t* env_rec_host, int servo, int hold, int window_rows, float inv_full, float v2_thresh, float track_tol);
int lm_replay_create_pd(lm_replay** out, struct lm_engine* h, const float* rec_host, const float* cmd_host, const int32_t* len_host,
                        int R, int T_max, const int32_t* env_rec_host, int cmd_mode, int hold, int window_rows,
                        float v2_thresh, float track_tol);
int lm_replay_steps(const lm_replay* p);
int lm_replay_update(lm_replay* p, int s, const float* obs, const float* rewards, float* record, float* actions_next, void* stream);
int lm_replay_destroy(lm_replay* p);

/* ---- PPO update (csrc/lm_ppo.hip): the loss and parameter gradient of one mini-batch of train/ppo.py PPO.update for the MLP policy above,
 * and GAE.  The optimiser, the gradient-norm clip, the KL-adaptive rate and the scalers stay with the caller.
 *
 * Flat parameter / gradient block, fp32, torch layout (row-major (out, in)), num_obs in {64, 88}:
 *   W1 (256, num_obs) | b1 (256) | W2 (128, 256) | b2 (128) | W3 (64, 128) | b3 (64) | Wm (12, 64) | bm (12) | Wv (1, 64) | bv (1) | log_std (12)
 * lm_mlp_grad_param_count(num_obs) is its length (58 649 / 64 793; -1 for another width).  It is read as it stands: no packing between
 * optimiser steps. */
int lm_mlp_grad_param_count(int num_obs);

typedef struct lm_ppo_hyper {
  float ratio_clip;       /* rc: the ratio is clamped to [1 - rc, 1 + rc] */
  float value_clip;       /* the value prediction moves at most this far from old_value_n */
  float value_scale;      /* factor on the value loss */
  float entropy_scale;    /* factor on the entropy term */
} lm_ppo_hyper;

/* With  mean, v = MLP(obs_n);  logp = sum_j [-1/2 ((a_j - mean_j) / exp(ls_j))^2 - ls_j - 1/2 ln 2 pi];  rl = logp - old_logp;  ratio = exp(rl):
 *   loss_pi = -mean_b min(adv ratio, adv clamp(ratio, 1 - rc, 1 + rc))
 *   vc = old_v + clamp(v - old_v, -value_clip, +value_clip);  loss_v = value_scale mean_b (ret - vc)^2
 *   ent = sum_j (ls_j + 1/2 + 1/2 ln 2 pi);  loss = loss_pi + loss_v - entropy_scale ent;  kl = mean_b ((ratio - 1) - rl)
 * grad [lm_mlp_grad_param_count] = d loss / d params, in the order of `params`;  stats [4] = loss_pi, loss_v, kl, ent.
 * Inputs, device fp32 contiguous: params (16-byte aligned), obs_n [B][num_obs] (normalised and clipped by the caller; 16-byte aligned),
 * actions [B][12], old_logp [B], old_value_n [B], adv [B], ret_n [B].  B is not padded by the caller: a ragged last tile is masked.
 * workspace: device memory, 16-byte aligned, at least lm_mlp_ppo_grad_workspace(num_obs, B) bytes (its contents on entry do not matter).
 * Every product runs as v_mfma_f32_16x16x4_f32 (exact fp32); no activation leaves the chip; two calls on the same inputs write the same
 * bits (per-workgroup partial sums in the workspace, added in a fixed order by a second kernel; no atomics).
 * Returns 0; LM_EINVAL (-1) for a null pointer, B < 1, num_obs not 64 / 88, a misaligned block, a workspace that is too small, or buffers
 * that are not memory of the calling thread's current device; -2 for a launch failure. */
int lm_mlp_ppo_grad(const float* params, const float* obs_n, const float* actions, const float* old_logp, const float* old_value_n,
                    const float* adv, const float* ret_n, int B, int num_obs, const lm_ppo_hyper* hp, float* grad, float* stats,
                    void* workspace, long long workspace_bytes, void* stream);
/* Bytes of workspace a call of that size needs (negative: the error code of lm_mlp_ppo_grad_geometry). */
long long lm_mlp_ppo_grad_workspace(int num_obs, int B);
/* The sample-tile size and the number of workgroups a call of that size launches on the current device: groups = min(tiles, compute
 * units), each workgroup looping over its tiles.  -2 without a device. */
int lm_mlp_ppo_grad_geometry(int num_obs, int B, int* tile, int* groups);

/* GAE(gamma, lambda) and returns in one launch, one lane per env, over a rollout plan's own buffers: rewards [T][N], values [T][N],
 * dones int64 [T][N], last_value [N] -> returns [T][N], advantages [T][N].  For t = T-1 .. 0, every operation rounded once, no contraction:
 *   nd = 1 - done;  delta = (r + (g32 next) nd) - v;  last = delta + (gl32 nd) last;  adv = last;  ret = adv + v;  next = v
 * with g32 = (float)gamma and gl32 = (float)(gamma * lam) (the double product, rounded once): bit for bit what distributed.compute_gae
 * computes in torch.  Returns 0, LM_EINVAL (null pointer, T < 1, N < 1) or -2. */
int lm_gae(const float* rewards, const float* values, const int64_t* dones, const float* last_value, int T, int N, double gamma, double lam,
           float* returns, float* advantages, void* stream);

/* ---- PPO update for the GNN policy (csrc/lm_gnn_ppo.hip): lm_mlp_ppo_grad with the network swapped (same loss, same lm_ppo_hyper, same
 * stats, same determinism and return codes; 64-wide observations only, as lm_gnn_forward).
 *
 * Flat parameter / gradient block, fp32, torch layout, in the order of the packed block of lm_gnn_param_count with the scaler rows left out
 * and log_std appended:
 *   input_layer1.weight (32,16) .bias (32) | input_layer2.weight (32,4) .bias (32) |
 *   3 x { linear1.weight (32,64) .bias (32) | linear2.weight (32,32) .bias (32) } |
 *   action_layer.weight (32) .bias (1) | value action_layer.weight (32) .bias (1) | log_std (12)
 * lm_gnn_grad_param_count() is its length (10 190).  It is read as it stands: no packing between optimiser steps.
 * mean, v = GraphPolicy(obs_n): the feature gather of create_features happens inside the kernel (columns 0..15 to node 0; columns 16 + idx,
 * 28 + idx, 40 + idx, 52 + idx with idx = 0 1 2 3 4 6 8 10 5 7 9 11 to the joint nodes 1..12; mean k is node k + 1).
 * Max aggregation: an exact tie among the messages into a node splits the gradient evenly among the tied edges (autograd's amax); an exact
 * tie in the value head's max over the nodes sends it to the lowest node index.
 * Inputs, workspace, grad and stats as for lm_mlp_ppo_grad.  Returns 0; LM_EINVAL (-1) for a null pointer, B < 1, a misaligned block, a
 * workspace that is too small (nothing is launched, nothing written), or buffers that are not memory of the calling thread's current device;
 * -2 for a launch failure. */
int lm_gnn_grad_param_count(void);
int lm_gnn_ppo_grad(const float* params, const float* obs_n, const float* actions, const float* old_logp, const float* old_value_n,
                    const float* adv, const float* ret_n, int B, const lm_ppo_hyper* hp, float* grad, float* stats, void* workspace,
                    long long workspace_bytes, void* stream);
long long lm_gnn_ppo_grad_workspace(int B);
int lm_gnn_ppo_grad_geometry(int B, int* tile, int* groups);

/* ---- the optimiser step of the PPO update (csrc/lm_optim.hip): gradient-norm clip + Adam on one flat fp32 block (the blocks above, or any
 * other), and the KL-adaptive learning rate, with the rate and the step count in device memory so that a caller's epoch loop never waits for
 * the host.
 *
 * State block: device double [LM_OPTIM_STATE] (lm_optim_state_len() returns the length), 8-byte aligned.  Slots:
 *   LM_OPTIM_LR the learning rate | LM_OPTIM_STEP Adam's step count | LM_OPTIM_GRAD_NORM, LM_OPTIM_CLIP_COEF of the last step |
 *   LM_OPTIM_KL the mean the last lm_kl_adaptive_lr call took | 5, 6: lr / (1 - beta1^step) and sqrt(1 - beta2^step) of the last step
 *   (derived by the step's first launch for its second) | 7 unused
 * It is double so that the rate walks through the very doubles the host rule produces.  lm_optim_state_init sets lr and step, clip_coef = 1
 * and the rest 0. */
#define LM_OPTIM_STATE 8
enum { LM_OPTIM_LR = 0, LM_OPTIM_STEP = 1, LM_OPTIM_GRAD_NORM = 2, LM_OPTIM_CLIP_COEF = 3, LM_OPTIM_KL = 4 };
int lm_optim_state_len(void);
int lm_optim_state_init(double* state, double lr, double step, void* stream);

typedef struct lm_optim_hyper {
  double beta1, beta2, eps;   /* Adam's (torch defaults 0.9, 0.999, 1e-8) */
  double max_norm;            /* the gradient-norm clip */
  int32_t clamp_offset;       /* entries [clamp_offset, clamp_offset + clamp_count) are floored at clamp_min after the step; */
  int32_t clamp_count;        /*   clamp_count 0: no floor (clamp_offset is then not read) */
  float clamp_min;
  int32_t reserved0;          /* 0 */
} lm_optim_hyper;

/* One optimiser step on params [n]: torch.nn.utils.clip_grad_norm_(max_norm, error_if_nonfinite = False) followed by torch.optim.Adam
 * (no weight decay, no amsgrad), with lr = state[LM_OPTIM_LR]:
 *   norm = ||grad||_2 over all n;  coef = min(1, max_norm / (norm + 1e-6));  g = coef grad;  step += 1
 *   m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2;  p -= (lr / (1 - beta1^step)) m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 *   p[e] = max(p[e], clamp_min) for e in the clamp range
 * evaluated per element in double and rounded once to fp32 per stored value (m, v, p); the squared norm is summed in double in an order fixed
 * by n.  grad is read only (it is not scaled in place).  step, grad_norm and clip_coef are left in state.  Non-finite gradients propagate as
 * they do in torch.  Two launches: one workgroup that writes state, then the step, which only reads it; no atomics; two calls on equal
 * inputs write equal bits.
 * params, grad, exp_avg, exp_avg_sq: device fp32 [n], 16-byte aligned (n itself is arbitrary: a scalar tail follows the 16-byte vectors).
 * Returns 0; LM_EINVAL (-1) for a null pointer, n < 1, a clamp range outside [0, n), a misaligned block, or buffers that are not memory of the
 * calling thread's current device - nothing is launched; -2 for a launch failure. */
int lm_adam_clip_step(float* params, const float* grad, float* exp_avg, float* exp_avg_sq, int n, double* state, const lm_optim_hyper* hyper,
                      void* stream);

/* The KL-adaptive rate of train/ppo.py PPO.update (skrl KLAdaptiveRL): kl_mean = the mean of kl [count] (device fp32, summed in double in
 * index order);  if threshold > 0:  kl_mean > 2 threshold: lr = max(lr / 1.5, lr_min);  else kl_mean < threshold / 2: lr = min(lr * 1.5, lr_max).
 * Writes state[LM_OPTIM_LR] and state[LM_OPTIM_KL] = kl_mean.  Returns as above (count < 1 is LM_EINVAL). */
int lm_kl_adaptive_lr(double* state, const float* kl, int count, double threshold, double lr_min, double lr_max, void* stream);

/* ---- the rest of a PPO iteration (csrc/lm_prepare.hip): the parameter pack of the forward kernels from the flat block the optimiser steps,
 * and the batch preparation of train/ppo.py PPO.update (both running scalers, the normalisation of observations, returns, old values and
 * advantages).  With them an iteration is a fixed sequence of launches that never waits for the host.  Every entry point validates on the host
 * before any launch - LM_EINVAL (-1) with an lm_last_error text for a null pointer, a size outside its set, a misaligned block, a workspace that
 * is too small, or buffers that are not memory of the calling thread's current device; nothing is launched and nothing written - and none of
 * them synchronises the device or allocates.  -2 for a launch failure.
 *
 * Scaler state: device double [2 C + 1] = mean (C) | var (C) | count, 8-byte aligned: the state of train/ppo.py RunningStandardScaler
 * (initially 0, 1, 1).  The value scaler's has C = 1.
 *
 * lm_mlp_pack_params: ONE launch.  flat = the block of lm_mlp_ppo_grad (num_obs 64 or 88); packed = the block of lm_mlp_forward_obs
 * (lm_mlp_param_count_obs(num_obs) words, 16-byte aligned), bit for bit what policies/mlp_model.py pack_mlp_params builds from the same
 * weights: hi / lo fp16 halves rounded to nearest even in the two K orders, 88 padded to 96, the head block with row 12 the value head and rows
 * 13..15 zero, biases, then the scaler rows  mean = float(state mean) | istd = 1 / (sqrt(float(var)) + float(eps)), every step the correctly
 * rounded fp32 result | clip.  scaler_state == NULL: mean 0, istd 1 and 3.0e38 in the clip word (eps and clip are then not read).
 * lm_gnn_pack_params: the same for the block of lm_gnn_forward (num_obs must be 64): the flat block of lm_gnn_ppo_grad without log_std,
 * followed by the mean row, the istd row and the clip word.
 * status: device int32.  The kernel ORs bits into it and never clears it (the caller zeroes it once): LM_PACK_NONFINITE a weight that is not
 * finite, LM_PACK_RANGE a finite weight with |w| >= 6.0e4 - the two conditions the torch packers raise on, over the tensors they check (the MLP's
 * four weight matrices; all of the GNN's block).  The content of packed after a flagged call is unspecified. */
enum { LM_PACK_NONFINITE = 1, LM_PACK_RANGE = 2 };
int lm_mlp_pack_params(const float* flat, int num_obs, const double* scaler_state, double eps, double clip, float* packed, int32_t* status,
                       void* stream);
int lm_gnn_pack_params(const float* flat, int num_obs, const double* scaler_state, double eps, double clip, float* packed, int32_t* status,
                       void* stream);

/* Batch statistics, ONE launch: obs [B][C] (16-byte aligned), ret [B], adv [B] (device fp32; C 64 or 88; B >= 2, because the unbiased deviation
 * of one sample is not a number) ->
 *   sums, device double [lm_ppo_batch_sums_len(C) = 2 C + 5]:  S obs_c (C) | S obs_c^2 (C) | S ret | S ret^2 | S adv | S adv^2 | B
 * All accumulation is in double in an order fixed by (B, C): per-workgroup partial sums in the workspace, then one pass over them in workgroup
 * order by the workgroup that finishes last (an integer ticket; no floating-point atomics).  Two calls write the same bits.
 * workspace: device memory, 16-byte aligned, at least lm_ppo_batch_stats_workspace(B, C) bytes.  Its first word is the ticket counter: it must
 * be 0 before the first call (a zeroed allocation) and every call leaves it 0; the rest may hold anything.  One workspace serves one stream. */
int lm_ppo_batch_sums_len(int C);
long long lm_ppo_batch_stats_workspace(int B, int C);
int lm_ppo_batch_stats(const float* obs, const float* ret, const float* adv, int B, int C, double* sums, void* workspace, long long workspace_bytes,
                       void* stream);

/* Merge and apply, TWO launches (one workgroup that writes the two states, then the apply, which only reads them).
 * Merge: n = sums[2 C + 4] samples into obs_state (C features; skipped when freeze_obs != 0) and val_state (1 feature, from S ret), with the
 * formula and the operation order of RunningStandardScaler.update, in double, no contraction:
 *   bmean = s / n;  bvar = max(ss / n - bmean bmean, 0) n / max(n - 1, 1);  delta = bmean - mean;  tot = count + n
 *   m2 = var count + bvar n + delta delta count n / tot;  mean = mean + delta n / tot;  var = m2 / tot;  count = tot
 * Apply, from the merged states, evaluated in double and rounded to fp32 once:
 *   obs_n = clamp((obs - mean) / (sqrt(var) + eps), -clip, +clip);  ret_n, old_val_n: the same with the value scaler
 *   adv_n = (adv - S adv / n) / (sqrt(max((S adv^2 - (S adv)^2 / n) / (n - 1), 0)) + 1e-8)          (the unbiased deviation, from the sums)
 * sums is read only, so a multi-rank caller can all-reduce it between lm_ppo_batch_stats and this call.  obs and obs_n 16-byte aligned;
 * inputs and outputs must not overlap. */
int lm_ppo_batch_apply(const float* obs, const float* ret, const float* old_val, const float* adv, int B, int C, const double* sums,
                       double* obs_state, double* val_state, int freeze_obs, double eps, double clip, float* obs_n, float* ret_n,
                       float* old_val_n, float* adv_n, void* stream);

#ifdef __cplusplus
}
#endif
#endif
