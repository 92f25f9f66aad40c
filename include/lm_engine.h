/*
 * lm_engine.h -- C ABI of the MI355X loco-manipulation physics-step engine (liblm_engine.so).
 *
 * The reference has no FFI on this path: the boundary is the Python object protocol
 *   VecEnvRLGames.step / reset / set_task      RobotLearning/omniisaacgymenvs/envs/vec_env_rlgames.py:48-90
 *   RLTask buffers + post_physics_step         RobotLearning/omniisaacgymenvs/tasks/base/rl_task.py:104-113,240-260
 * below which it calls closed-source PhysX (World.step, ArticulationView / RigidPrimView tensor API,
 * vec_env_rlgames.py:65; robot/base/robot.py:276-321,357-461; objects/base/rigid_object.py:30-58).
 * These entry points are what a binding for that path binds instead (INTEGRATION.md shows the ctypes
 * stub).  Plain pointers and sizes only; no torch types; no exceptions cross the ABI; every call
 * returns 0 on success or a negative LM_E* code (lm_last_error() gives the text).
 *
 * Memory: all device buffers are owned by the handle (hipMalloc) and exposed through lm_ptr();
 * output buffers for step() are caller-provided device pointers (so a host binding can hand out
 * fresh tensors per step, matching the "returned tensors are clones" contract of
 * vec_env_rlgames.py:41-46 without extra copy kernels).  The stream is the caller's.
 */
#ifndef LM_ENGINE_H
#define LM_ENGINE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LM_OK 0
#define LM_EINVAL (-1)
#define LM_EHIP (-2)
#define LM_ENOMEM (-3)

#define LM_MODE_LOCO 0   /* free base on a ground plane   (QuadrupedPoseControl)      */
#define LM_MODE_MANI 1   /* fixed inverted base + plate    (QuadrupedManipulatePlate)  */

#define LM_STATE_ROWS 115  /* float state, SoA [row][N]: see DESIGN.md 4.1 */
#define LM_CNT_ROWS 6      /* int64 counters, SoA [row][N] */
#define LM_NUM_OBS 64        /* velocity-drive tasks; the custom-controller tasks have 88 (lm_num_obs) */
#define LM_MAX_OBS 88
#define LM_TERM_ROWS 11
#define LM_NUM_STATES 93
#define LM_NUM_ACTIONS 12
#define LM_NUM_EXTRAS 13  /* 7 reward-term means, success_rate, success_rate of task 0 / task 1 (co-train),
                             custom-controller means: mechanical_power, position_target_error, rot_dist_decreasing */
#define LM_TABLE_FLOATS 502  /* 10 hub + 4 x 123 limb (RobotModel.packed_table) */
/* Bumped whenever lm_params, the table layout or the meaning of an entry point changes.  Every lm_params block carries it together with the
 * caller's sizeof(lm_params) and LM_TABLE_FLOATS (first three fields); lm_create returns LM_EINVAL when any of them differs from what the
 * library was built with, instead of reading a shifted struct or past the end of a shorter table.
 *   1  round 1     2  round 2 (drive_mode, 502-float table; not stamped)     3  round 3 (the stamp itself; pgs_iters per contact surface)
 *   4  round 3 (pd_second_pass replaces sat_probe: the PD-actuator families decide their clamp on the pre-step state, one pass)
 *   5  contact-material randomisation (dr_mat, dr_mat_buckets, mat_mu_robot / mat_mu_other, friction_combine, friction_scale; LM_DR_PHYS_ROWS 43) */
#define LM_ABI_VERSION 5

/* Task / simulation constants for one task family.  Mirrors EngineParams (engine_config.py);
 * sources in the reference are cited there. */
/* Domain randomisation.  One channel = one entry of the YAML block cfg/task/QuadrupedPoseControl.yaml:116-173
 * (operation / distribution / distribution_parameters [/ frequency_interval]).  Observation and action noise follow
 * utils/domain_randomization/randomize.py:212-306 (wrapper call sites vec_env_rlgames.py:56-58,70-72); the physics attributes are
 * sampled per env inside lm_step (the reference delegates them to omni.replicator.isaac; semantics in DESIGN.md 3.6). */
#define LM_DR_CHANNELS 9
enum { LM_DR_OBS_RESET = 0, LM_DR_OBS_INTERVAL = 1, LM_DR_ACT_RESET = 2, LM_DR_ACT_INTERVAL = 3,
       LM_DR_GRAVITY = 4, LM_DR_BASE_FORCE = 5, LM_DR_MAX_EFFORT = 6, LM_DR_MAX_VELOCITY = 7,
       LM_DR_JOINT_DAMPING = 8 /* articulation `damping` of the PD-actuator tasks (variants 1 / 2): scales joint_damping */ };
enum { LM_DR_ADDITIVE = 0, LM_DR_SCALING = 1, LM_DR_DIRECT = 2 };
enum { LM_DRIVE_VELOCITY = 0, LM_DRIVE_POSITION = 1, LM_DRIVE_EFFORT = 2 };
enum { LM_DR_GAUSSIAN = 0, LM_DR_UNIFORM = 1, LM_DR_LOGUNIFORM = 2 };
typedef struct lm_dr_channel {
  int32_t enabled;
  int32_t operation;       /* LM_DR_ADDITIVE / SCALING / DIRECT */
  int32_t distribution;    /* LM_DR_GAUSSIAN / UNIFORM / LOGUNIFORM */
  int32_t interval;        /* frequency_interval of an on_interval entry (>= 1); 0 = on_reset entry */
  float p0[3], p1[3];      /* distribution_parameters: mean / std or low / high (one pair per component for gravity and force) */
} lm_dr_channel;
/* Contact-material channels: articulation_views.<robot>.material_properties (the feet, the robot's only colliders) and
 * rigid_prim_views.plate.material_properties.  p0 / p1 components are [static, dynamic, restitution]; only the dynamic one enters, because the
 * contact solver has one Coulomb coefficient.  interval: >= 1 on_interval, 0 on_reset (gated by dr_min_frequency like the attributes above),
 * LM_DR_ON_STARTUP: one draw per env, keyed by (seed, channel, env) only.  Per env and step
 *   mu_env = max(0, friction_scale * combine(robot, other))
 * where robot / other are mat_mu_robot / mat_mu_other after their channel's draw (other = the ground in locomotion blocks, the plate in
 * manipulation blocks).  With both channels off the block's `mu` is used unchanged. */
#define LM_DR_MATERIALS 2
enum { LM_DR_MAT_ROBOT = 0, LM_DR_MAT_OTHER = 1 };
#define LM_DR_ON_STARTUP (-1)
enum { LM_COMBINE_AVERAGE = 0, LM_COMBINE_MIN = 1, LM_COMBINE_MULTIPLY = 2, LM_COMBINE_MAX = 3 };      /* PhysX's PxCombineMode order */
#define LM_DR_PHYS_ROWS 43
#define LM_DR_PHYS_MU 42   /* row of mu_env (the Coulomb coefficient the contact solve of the last step used) */
#define LM_DR_CNT_ROWS 5   /* int64 [row][N]: observation noise counter, action noise counter, dr_step, randomization_buf, dr_reset_key */
/* Reset-state channels: the state an env is reset to, drawn inside lm_step at the moment of the reset.  They live in a struct of
 * their own, handed over with lm_set_reset_randomization, so that lm_params keeps its layout.  on_reset only (interval 0).  A reset that passes
 * the dr_min_frequency gate draws, keyed by (seed, stream, env, new episode number, component); one that does not resets to the nominal state.
 *   LM_DR_RESET_JOINT_POS     12 components (one draw per driven joint, scalar parameters p0[0] / p1[0]) on init_q
 *   LM_DR_RESET_JOINT_VEL     12 components, scalar parameters, on the nominal 0: additive or direct
 *   LM_DR_RESET_POSITION      3 components, per-component parameters, on the free body's nominal position
 *   LM_DR_RESET_ORIENTATION   3 Euler angles (roll, pitch, yaw), per-component parameters, turned into a quaternion q_draw:
 *                             direct: q = q_draw; additive: q = q_draw (x) q_nominal (applied in the world frame after the nominal one)
 * The free body is the base in locomotion blocks and the plate in manipulation blocks.  No clamping to the joint ranges: a draw outside
 * d1_rst / d23_rst makes the env reset again on the next step.  The random streams are 12..15 (after the material streams 10, 11). */
#define LM_DR_RESET_CHANNELS 4
enum { LM_DR_RESET_JOINT_POS = 0, LM_DR_RESET_JOINT_VEL = 1, LM_DR_RESET_POSITION = 2, LM_DR_RESET_ORIENTATION = 3 };
typedef struct lm_reset_dr { lm_dr_channel ch[LM_DR_RESET_CHANNELS]; } lm_reset_dr;
#define LM_DR_RESET_ROWS 31  /* float [row][N]: q 12, qd 12, free-body position 3, free-body quaternion (w, x, y, z) 4 */
/* Mass channels: per-env masses of the plate and of the robot's 21 bodies, drawn inside lm_step for the control step (constant
 * over its sub-steps).  They live in a struct of their own, handed over with lm_set_mass_randomization, so that lm_params keeps its layout.
 * interval: >= 1 on_interval, 0 on_reset (gated by dr_min_frequency; nominal before the first gated reset), LM_DR_ON_STARTUP: one draw per env,
 * keyed by (seed, stream, env, component) only.  Scalar parameters p0[0] / p1[0] for the two plate channels; the body channel reads body_p0 /
 * body_p1, one pair per body in TABLE ORDER: 0 = hub, 1 + 5 limb + j with j over (shell, link4, link3, link1, link2); that index is also the
 * component of the draw.
 *   LM_DR_MASS_PLATE          the plate's mass.  Mass only: COM and inertia about the COM stay (what setting a mass through a simulator's tensor
 *                             API does); the spatial inertia about the plate origin changes through the parallel-axis term
 *   LM_DR_MASS_PLATE_DENSITY  a factor s on the plate's mass AND its inertia about the COM; LM_DR_ON_STARTUP + LM_DR_SCALING only (the URDF gives
 *                             mass and inertia but no volume: no nominal density exists).  Applied first: the nominal of LM_DR_MASS_PLATE is then
 *                             s x plate_mass
 *   LM_DR_MASS_BODIES         21 components, the masses of the hub and the limb bodies; mass only, as above
 * A drawn mass (and s) is floored at LM_DR_MASS_FLOOR x its nominal, so that a gaussian tail cannot produce a non-positive mass; a bounded
 * distribution (uniform, loguniform) whose range reaches a non-positive mass is refused by lm_set_mass_randomization.  The plate channels exist
 * on manipulation blocks only; in a manipulation block the base is fixed, so the hub's draw is recorded but has no effect.  The random streams
 * are 16 (plate mass), 17 (plate density), 18 (body masses). */
#define LM_DR_MASS_CHANNELS 3
enum { LM_DR_MASS_PLATE = 0, LM_DR_MASS_PLATE_DENSITY = 1, LM_DR_MASS_BODIES = 2 };
#define LM_NUM_BODIES 21
#define LM_DR_MASS_FLOOR 0.05f
typedef struct lm_mass_dr { lm_dr_channel ch[LM_DR_MASS_CHANNELS];
                            float body_p0[LM_NUM_BODIES], body_p1[LM_NUM_BODIES]; /* table order */ } lm_mass_dr;
#define LM_DR_MASS_ROWS 23   /* float [row][N]: plate mass, plate inertia factor, 21 body masses (table order): what the last step used, floored */
/* Actuator channels: per-env drive gains and command latency, drawn inside lm_step for the control step.  They live in a
 * struct of their own, handed over with lm_set_actuator_randomization, so that lm_params keeps its layout.  interval as for the mass channels
 * (>= 1 on_interval, 0 on_reset behind dr_min_frequency and nominal before the first gated reset, LM_DR_ON_STARTUP).  One draw per env
 * (component 0, scalar parameters p0[0] / p1[0]); the random streams are 19, 20, 21.
 *   LM_DR_ACTUATOR_KP       the position gain of the 12 driven joints, nominal pd_kp.  Variants 1 / 2, and variant 0 in LM_DRIVE_POSITION; there is
 *                      no position gain in LM_DRIVE_VELOCITY / LM_DRIVE_EFFORT
 *   LM_DR_ACTUATOR_KD       the velocity gain, nominal kd: the implicit drive damping, the saturation test and the drive torque all use the env's
 *                      value, and kp / kd is formed per env from the two draws.  Every family except LM_DRIVE_EFFORT (gains off)
 *   LM_DR_ACTUATOR_LATENCY  command latency in sub-steps, nominal 0, additive or direct: d = clamp(floor(draw), 0, substeps).  In the first d
 *                      sub-steps of the control step the PD law follows the PREVIOUS command (the swing / extension targets before this step's
 *                      action was integrated; init_se on a resetting env), from sub-step d on the new one; d = substeps delays the command by a
 *                      whole control period.  What the task layer reads (the stored targets, the target-error terms, the logged torque - the
 *                      torque that was applied -, acc_substeps) is unchanged.  Variants 1 / 2 only
 * A drawn gain is floored at LM_DR_MASS_FLOOR x its nominal (kd must stay positive: the solve uses kp / kd); a uniform / log-uniform range
 * that reaches a non-positive gain is refused.  One kp and one kd per env, not per joint: that is what the CPU oracle can check. */
#define LM_DR_ACTUATOR_CHANNELS 3
enum { LM_DR_ACTUATOR_KP = 0, LM_DR_ACTUATOR_KD = 1, LM_DR_ACTUATOR_LATENCY = 2 };
typedef struct lm_actuator_dr { lm_dr_channel ch[LM_DR_ACTUATOR_CHANNELS]; } lm_actuator_dr;
#define LM_DR_ACTUATOR_ROWS 3   /* float [row][N]: kp, kd, latency d (sub-steps) the last step used */

/* Contact-force reporting, opt-in per engine with lm_enable_contact_forces.  The record is float [LM_CONTACT_ROWS][N]:
 *   rows 3*l + c   force on foot l (limb order of the state, 0..3) BY THE OTHER SURFACE - the ground in locomotion blocks, the plate in
 *                  manipulation blocks - component c (x, y, z) in the WORLD frame, in newtons, averaged over the sub-steps of the launch:
 *                    F_l = 1 / (n_sub dt) * sum over the sub-steps of  R_b (lam_n C0 + lam_1 C1 + lam_2 C2)
 *                  lam = the impulses the contact solve returned in the LAST pass of that sub-step (the second drive pass where it runs),
 *                  C0, C1, C2 = that sub-step's contact axes in hub coordinates, R_b = the base's orientation (the fixed one in manipulation
 *                  blocks).  In the world frame the axes are: locomotion n = (0, 0, 1), t1 = the base's x axis projected onto the ground and
 *                  normalised, t2 = n x t1; manipulation n = sg x (plate z axis), pointing from the plate to the robot's side, t1 = the plate's
 *                  x axis, t2 = n x t1 (the kernels evaluate the sum in this form).  Neither clamped nor filtered
 *   rows 12 + l    contact fraction of foot l: the share of those sub-steps with lam_n > 0, a multiple of 1 / n_sub
 * n_sub = the sub-steps the launch ran: params.substeps for lm_step, n for lm_substeps(h, targets, n); lm_post_physics (no sub-step) and
 * lm_substeps(.., 0) leave the record as it was.  An env that lm_step resets reports the sub-steps after its reset (all of them).  The record
 * is a derived output of the last launch, not state: nothing reads it back, and a checkpoint (Engine.state_dict) does not carry it. */
#define LM_CONTACT_ROWS 16

/* Per-env physics parameters held by the caller, opt-in per engine with lm_enable_env_params.  The hold table is
 * float [LM_ENV_PARAM_ROWS][N]: the three records one after the other,
 *   rows [0, 43)    as LM_PTR_DR_PHYS      max efforts 12, max joint velocities 12, gravity 3, base force 3, joint damping 12, mu_env 1
 *   rows [43, 66)   as LM_PTR_DR_MASS      plate mass, plate inertia factor, 21 body masses (table order)
 *   rows [66, 69)   as LM_PTR_DR_ACTUATOR  kp, kd, command latency in sub-steps
 * with a row mask beside it (lm_env_params_held).  A row is held for ALL envs of the engine or for none, so the switches of the step stay uniform
 * over a wavefront.  In every lm_step of such an engine the value of a held row replaces what the row's channel produced (or the nominal value,
 * with the channel off), after the channels have drawn and before the records are written: the records report the held values.  A held value is
 * used exactly as stored - no floor (lm_set_env_params validated it), no re-derivation: the held plate mass is the mass whatever the inertia
 * factor, and a held mu row IS mu_env, the coefficient the contact solve uses, after friction_scale and the combine mode.  What the drawing path
 * derives is derived the same way: kp / kd from whichever of the two are held or drawn; the body-mass and plate paths of the sub-step go on when
 * one of their rows is held, as they do when their channel is on.  On a co-training engine the plate rows act on the manipulation block only.
 * Not combined yet (follow-ups): contact-force reporting (each of lm_enable_env_params / lm_enable_contact_forces(h, 1) is refused while the
 * other is on) and the staged entry points, which refuse every randomised engine. */
#define LM_ENV_PARAM_ROWS (LM_DR_PHYS_ROWS + LM_DR_MASS_ROWS + LM_DR_ACTUATOR_ROWS)   /* 69 */
#define LM_ENV_PARAM_MASS_ROW0 LM_DR_PHYS_ROWS                          /* 43 */
#define LM_ENV_PARAM_ACTUATOR_ROW0 (LM_DR_PHYS_ROWS + LM_DR_MASS_ROWS)  /* 66 */

typedef struct lm_params {
  int32_t abi_version;     /* LM_ABI_VERSION of the header the caller was compiled against */
  int32_t params_size;     /* the caller's sizeof(lm_params) */
  int32_t table_floats;    /* the caller's LM_TABLE_FLOATS = the length of the table it passes to lm_create */
  int32_t reserved0;       /* 0 */
  float dt, kd, tau_max, act_scale, mu, tip_radius, baumgarte, max_depen_vel, max_joint_vel, gravity;
  int32_t substeps, pgs_iters, mode;
  float fixed_base_pos[3], fixed_base_quat[4];
  float plate_mass, plate_com[3], plate_inertia[3], plate_half[3], plate_center[3];
  float init_q[12], init_base_pos[3], init_base_quat[4], init_plate_pos[3], init_plate_quat[4];
  float default_tip[12], goal_lo[3], goal_hi[3];
  float s_pos, s_lin, s_ang, s_q, s_qd;
  float quat_scale, rot_eps, trans_scale, acc_scale, rate_scale, bonus, limit_pen, fall_pen, succ_thresh;
  int32_t max_consec, max_episode;
  float d23_pen[2], d23_rst[2], d1_pen[4][2], d1_rst[4][2];
  float h_base, h_corner, h_knee, corner[4][3];
  float clip_obs, clip_actions;
  int32_t max_reset_counts;
  /* custom-controller task family (quadruped_pose_control_custom_controller.py:24-52,88-97,255-307) */
  int32_t variant;           /* 0 velocity-drive tasks, 1 custom-controller tasks, 2 position-control tasks (same PD actuator and swing/extension
                                actions; 64-wide observation with the scaled joint targets in place of the actions; reward of variant 0;
                                quadruped_pose_control_position_control.py:24-118,438-455, joint_locomanipulation_position_control.py:37-44,365-408) */
  int32_t num_obs;           /* 64 / 88 */
  float pd_kp, joint_damping, act_scale_se;
  float se_lo[12], se_hi[12], init_se[12];
  float torque_div, power_scale, target_err_scale, rot_dec_scale, rot_dec_thresh;
  int32_t cc_update_last_tgt;
  int32_t acc_substeps;      /* variants 1/2: trailing sub-steps the joint acceleration spans (controlFrequencyInv; robot.py:289-291) */
  int32_t dr_enabled;        /* domain_randomization.randomize */
  int32_t dr_min_frequency;  /* domain_randomization.min_frequency: gate of the on_reset physics attributes (quadruped_pose_control.py:224-228) */
  lm_dr_channel dr[LM_DR_CHANNELS];
  int32_t drive_mode;        /* variant 0 only - RobotOmni.take_action's control modes (robot/base/robot.py:444-461):
                                LM_DRIVE_VELOCITY  target = a * act_scale [rad/s]           implicit damper kd (the mode every task of the path uses)
                                LM_DRIVE_POSITION  target = a * act_scale [rad] (act_scale = pi); tau = pd_kp (q* - q) - kd qd, re-evaluated per sub-step
                                LM_DRIVE_EFFORT    tau = a * act_scale [N m] (act_scale = torque limit), gains off */
  int32_t pd_second_pass;    /* variants 1 / 2.  0 (default): which joints sit on the +-tau_max limit is decided from the PD torque on the state BEFORE
                                the sub-step, as the reference's explicit clamp decides it (quadruped_pose_control_custom_controller.py:289-293); the others
                                get the implicit form of the law in ONE pass, and the 0.02 % of joint-sub-steps whose implicit torque then leaves the
                                limit keep it.  1: those joints are put on the limit too and the sub-step is solved a second time (the applied
                                torque never exceeds tau_max; a step then takes as long as its slowest wavefront: +6 us at 4096 envs).  DESIGN.md 3.3 */
  /* contact-material randomisation (ABI 5; see LM_DR_MATERIALS above).  Read by the randomised kernels only, when dr_enabled */
  lm_dr_channel dr_mat[LM_DR_MATERIALS];   /* LM_DR_MAT_ROBOT, LM_DR_MAT_OTHER; interval LM_DR_ON_STARTUP / 0 / >= 1 */
  int32_t dr_mat_buckets[LM_DR_MATERIALS]; /* num_buckets: 0 = continuous; K >= 1: the channel's uniform variate is quantised to K levels first */
  float mat_mu_robot, mat_mu_other;        /* nominal dynamic coefficients of the feet and of the other surface (ground / plate) */
  int32_t friction_combine;                /* LM_COMBINE_* */
  float friction_scale;                    /* effective / nominal coefficient (engine_config.FRICTION_SCALE) */
  /* derived by lm_create (callers leave zero) */
  float plate_si[10];      /* plate spatial inertia about its origin */
  float plate_phi[36];     /* its inverse */
  float ctrl_dt_inv, acc_dt_inv;
} lm_params;

typedef struct lm_engine lm_engine;   /* opaque */

/* Pointers the host side may wrap zero-copy.  LM_PTR_OBS_BUF, LM_PTR_STATES_BUF and LM_PTR_TERMS are the engine's own unclipped copies of
 * what lm_step's out_obs / out_states deliver clipped: lm_step keeps each of them current from the first lm_ptr() call for it on (ask before
 * the step whose values you want), and in any case when the matching out_* argument is NULL; a caller that only consumes the out_* buffers
 * does not pay for the second copy.  The staged entry points (lm_post_physics ...) always write them.
 * CAVEATS of the on-demand copies: (1) the first lm_ptr() call for one of the three changes what LATER lm_step launches write - the buffer it
 * returns is zeros / an older step's values until the next step (the Python mirror warns when a view is first requested after stepping);
 * (2) a hipGraph the CALLER captured around lm_step before that first lm_ptr() call keeps the kernel arguments of capture time (NULL view
 * pointers) for ever: request the views you need before capturing.  lm_rollout's own graph is re-captured when the set of views changed. */
typedef enum {
  LM_PTR_STATE = 0,     /* float [LM_STATE_ROWS][N]                                  */
  LM_PTR_CNT = 1,       /* int64 [LM_CNT_ROWS][N]: successes, consecutive_successes,
                           goal_reset_buf, reset_buf, progress_buf, episode_count    */
  LM_PTR_OBS_BUF = 2,   /* float [N][lm_num_obs()]  task.obs_buf (unclipped)   rl_task.py:107  */
  LM_PTR_STATES_BUF = 3,/* float [N][93]  task.states_buf                            */
  LM_PTR_REW_BUF = 4,   /* float [N]      task.rew_buf                               */
  LM_PTR_EXTRAS = 5,    /* float [LM_NUM_EXTRAS]  reward-term means + success rates     */
  LM_PTR_STATS = 6,     /* int64 [6] {num_successes, num_resets} x {all, task 0, task 1}; float [3] rates at byte 48;
                           uint32 at byte 60: envs whose state became non-finite / exploded and was replaced by the reset pose */
  LM_PTR_TERMS = 7,     /* float [LM_TERM_ROWS][N]  per-env reward terms of the last step */
  LM_PTR_DR_CNT = 8,    /* int64 [LM_DR_CNT_ROWS][N]  domain-randomisation counters */
  LM_PTR_DR_PHYS = 9,   /* float [LM_DR_PHYS_ROWS][N]  attributes sampled for the last step: max efforts 12, max joint velocities 12,
                           gravity 3, base force 3, joint damping 12, mu_env 1 (row LM_DR_PHYS_MU) */
  LM_PTR_DR_RESET_STATE = 10, /* float [LM_DR_RESET_ROWS][N]  the state each env was last reset to by lm_step (nominal resets included);
                           randomised engines only (NULL otherwise) */
  LM_PTR_DR_MASS = 11,  /* float [LM_DR_MASS_ROWS][N]  plate mass, plate inertia factor and the 21 body masses (table order) the last step used;
                           the nominal values until a mass channel draws; randomised engines only (NULL otherwise) */
  LM_PTR_CONTACT = 12,  /* float [LM_CONTACT_ROWS][N]  per-foot contact forces and contact fractions of the last reporting launch; NULL until
                           lm_enable_contact_forces(h, 1).  One more row of N floats follows it, all bits set, which no kernel writes (a guard
                           the tests read) */
  LM_PTR_DR_ACTUATOR = 13,/* float [LM_DR_ACTUATOR_ROWS][N]  kp, kd and the command latency d (sub-steps) the last step used; the nominal values
                           (pd_kp, kd, 0) until an actuator channel draws; randomised engines only (NULL otherwise) */
  LM_PTR_ENV_PARAMS = 14  /* float [LM_ENV_PARAM_ROWS][N]  the hold table of lm_enable_env_params (NULL until then).  Read it freely; write it
                           through lm_set_env_params, which validates and sets the mask */
} lm_ptr_kind;

/* Create an engine for n_envs environments on the current HIP device.
 *   table      : LM_TABLE_FLOATS packed robot model (host pointer)
 *   params     : n_tasks (1 or 2) parameter blocks (host pointer); with 2 tasks, envs [0, split_env)
 *                use params[0] and [split_env, n_envs) use params[1] (co-train layout,
 *                joint_locomanipulation.py:25-34); split_env must be a multiple of 16.
 *   seed       : stream seed of the in-kernel goal sampler (replaces torch.rand in utils/math.py:184)
 * n_envs must be positive and below 2^25 (33 554 432) per engine: the width of the reset counts in the fused extras reduction; LM_EINVAL otherwise.
 * All envs start with reset_buf = 1 (rl_task.py:111).
 * The engine belongs to the device that is current in the calling thread here: every later call on the handle must be made with the
 * same device current (one process per GPU) and returns LM_EINVAL otherwise instead of launching on another GPU. */
int lm_create(lm_engine** out, int n_envs, const float* table, const lm_params* params, int n_tasks,
              int split_env, uint32_t seed);
int lm_destroy(lm_engine* h);

/* Reset-state randomisation of parameter block `block` (0, or 1 on a two-task engine): validates *rd and copies it to device memory owned
 * by the handle; later lm_step launches draw from it (see LM_DR_RESET_CHANNELS above).  All four channels are off after lm_create.
 * LM_EINVAL: engine without dr_enabled; block out of range; an enabled channel with a bad operation / distribution, an interval other
 * than 0 (on_reset is the only trigger), `scaling` on the joint velocities (nominal 0) or on the orientation (a quaternion is not scaled),
 * log-uniform with non-positive bounds, or non-finite parameters.  Synchronous (a blocking copy): call it before the first step and not
 * while a graph that contains lm_step is being captured. */
int lm_set_reset_randomization(lm_engine* h, int block, const lm_reset_dr* rd);

/* Mass randomisation of parameter block `block` (0, or 1 on a two-task engine): validates *md and copies it to device memory owned by the
 * handle; later lm_step launches draw from it (see LM_DR_MASS_CHANNELS above).  All three channels are off after lm_create.
 * LM_EINVAL: engine without dr_enabled; block out of range; an enabled channel with a bad operation / distribution / interval (below
 * LM_DR_ON_STARTUP); the density channel with anything but LM_DR_ON_STARTUP + LM_DR_SCALING; non-finite parameters; log-uniform with
 * non-positive bounds; a uniform / log-uniform range that reaches a non-positive mass (or density factor); a plate channel on a locomotion
 * block.  Synchronous (a blocking copy): call it before the first step and not while a graph that contains lm_step is being captured. */
int lm_set_mass_randomization(lm_engine* h, int block, const lm_mass_dr* md);

/* Actuator randomisation of parameter block `block` (0, or 1 on a two-task engine): validates *ad and copies it to device memory owned by
 * the handle; later lm_step launches draw from it (see LM_DR_ACTUATOR_CHANNELS above).  All three channels are off after lm_create.
 * LM_EINVAL: engine without dr_enabled; block out of range; an enabled channel with a bad operation / distribution / interval (below
 * LM_DR_ON_STARTUP); non-finite parameters; log-uniform with non-positive bounds; a uniform / log-uniform range that reaches a non-positive
 * gain; LM_DR_ACTUATOR_KP on a variant-0 block that is not in LM_DRIVE_POSITION; LM_DR_ACTUATOR_KD on a block in LM_DRIVE_EFFORT; LM_DR_ACTUATOR_LATENCY on
 * a variant-0 block, or with LM_DR_SCALING (the nominal is 0).  Synchronous (a blocking copy): call it before the first step and not while a
 * graph that contains lm_step is being captured. */
int lm_set_actuator_randomization(lm_engine* h, int block, const lm_actuator_dr* ad);

/* Contact-force reporting on (on != 0) or off (0, the state after lm_create); see LM_CONTACT_ROWS.  The first enable allocates the record
 * and zeroes it; later calls only flip the switch (the record keeps its contents while reporting is off: nothing writes it then).
 * With reporting on, lm_step and lm_substeps launch builds of their kernels that also write the record (k_step_cf, k_step_pd_cf,
 * k_step_dr_cf, k_step_dr_pd_cf, k_substeps_cf: every family, both blocks of a co-training engine) - still one launch, no atomics; with it off
 * they launch exactly the kernels they launched before this entry point existed.  An un-randomised locomotion engine above the k_step_w2
 * threshold (see lm_step) runs the one-wavefront reporting kernel while reporting is on: the two-wavefront build does not report.
 * Rollouts (lm_policy.h): LM_ROLLOUT_PERSISTENT returns -1 while reporting is on (the persistent kernel does not report), LM_ROLLOUT_AUTO
 * picks the graph, LM_ROLLOUT_ENQUEUE and LM_ROLLOUT_GRAPH leave the LAST step's record in the buffer.  A rollout plan created before the
 * switch stays valid: its graph is re-captured on the next run, as after lm_set_seed, so the switch is never refused on account of a plan.
 * A hipGraph the CALLER captured around lm_step keeps the kernel of capture time.
 * LM_EINVAL: null handle, the calling thread's current device is not the engine's, or on != 0 on an engine with env params enabled
 * (lm_enable_env_params; combining the two is a follow-up).  Synchronous (allocation, blocking clear): not to be called while a graph that
 * contains lm_step is being captured. */
int lm_enable_contact_forces(lm_engine* h, int on);

/* Per-env parameters held by the caller (see LM_ENV_PARAM_ROWS).  lm_enable_env_params allocates the hold table and its mask with nothing
 * held; from then on lm_step launches builds of the randomised kernels that apply the holds (k_step_dr_hp, k_step_dr_pd_hp: one launch, as
 * before); an engine that never enables launches exactly the kernels it launched before this entry point existed.  There is no way back.
 * Rollouts (lm_policy.h): LM_ROLLOUT_AUTO / GRAPH / ENQUEUE work (LM_ROLLOUT_PERSISTENT refuses every randomised engine); a plan created before
 * the call stays valid: its graph is re-captured on the next run.  Holding, changing or clearing rows afterwards needs no re-capture: table
 * and mask live in device memory.  A hipGraph the CALLER captured around lm_step keeps the kernel of capture time.
 * LM_EINVAL: null handle; the calling thread's current device is not the engine's; an engine created without dr_enabled (the un-randomised
 * kernels carry no per-env parameters: create the engine with dr_enabled and no channel on); contact-force reporting on.  Synchronous
 * (allocation, blocking clear), like lm_enable_contact_forces. */
int lm_enable_env_params(lm_engine* h);
/* Hold rows [row0, row0 + nrows) at values_host, a HOST float [nrows][N].  Everything is validated on the host before anything is copied;
 * a refused call leaves table and mask as they were.  LM_EINVAL: null argument; not enabled; foreign device; rows outside the table; a value
 * that is not finite; a mass, the plate's inertia factor, kp or kd that is not > 0; mu, a max effort, a max joint velocity or a joint damping
 * that is < 0; a latency that is not whole or outside [0, substeps] of a block that reads it; a row that no block of the engine reads: kp
 * without a position gain (variant 0 in velocity or effort drive), kd in effort drive, latency on variant 0, the plate rows on an engine
 * without a manipulation block.
 * SYNCHRONOUS against the whole device: after the validation the call waits for the device (hipDeviceSynchronize) before it touches the table or
 * the mask, and its copies are blocking.  When it returns, every lm_step enqueued before it - on any stream, the caller's non-blocking ones
 * included - has run with the rows as they were, and every later one sees the new rows.  Not to be called while a graph that contains lm_step
 * is being captured (like lm_enable_env_params); a graph captured before it needs no re-capture. */
int lm_set_env_params(lm_engine* h, int row0, int nrows, const float* values_host);
/* Rows [row0, row0 + nrows) follow their channel - or the nominal value - again from the next step on.  A mass / actuator record row that no
 * channel writes shows the nominal value again.  Synchronous against the whole device in the same way as lm_set_env_params: it waits for the
 * device before it changes the mask or rewrites a record row, so steps enqueued before it still run with the rows held. */
int lm_clear_env_params(lm_engine* h, int row0, int nrows);
/* mask_out[0] bit r: row r (< 64) is held; mask_out[1] bit r - 64: row r.  LM_EINVAL: null argument, or not enabled. */
int lm_env_params_held(const lm_engine* h, uint64_t* mask_out);

/* One VecEnvRLGames.step(): reset flagged envs, clamp + apply actions, controlFrequencyInv physics
 * sub-steps, observations / reward / termination.  (vec_env_rlgames.py:56-79)
 *   actions     device float [N][12]
 *   goal_rand   device float [N][3] uniforms for goal sampling, or NULL for the in-kernel hash RNG
 *   out_*       device buffers receiving clipped copies for the caller (any may be NULL; see lm_ptr_kind for the unclipped copies):
 *               obs [N][lm_num_obs], states [N][93], rew [N], resets int64 [N], extras float [LM_NUM_EXTRAS]
 *   stream      hipStream_t (void* here so the header needs no HIP include)
 * With params.dr_enabled the same launch also applies the action noise (before the clamp), samples this step's physics attributes
 * and adds the observation noise (obs_buf and out_obs); the staged entry points below refuse a randomised engine.
 * One kernel launch.  Un-randomised velocity-drive locomotion engines of more than 32 768 envs get the build of the same kernel for two
 * wavefronts per SIMD (k_step_w2: same bits, faster beyond two generations of workgroups; the environment variable LM_W2_MIN_ENVS, read
 * by lm_create, moves that threshold).  Un-randomised velocity-drive engines with a locomotion block, small enough that two wavefronts per
 * 16 envs still find a SIMD each (8192 envs on MI355X), get the kernel with a helper wavefront per workgroup (k_step_h2: same bits; the
 * environment variable LM_H2_MAX_ENVS, read by lm_create, moves that threshold, 0 = never).  Up to one workgroup per compute unit
 * (4096 envs on MI355X) the same engines get the kernel with two helper wavefronts (k_step_h3: same bits; LM_H3_MAX_ENVS moves that
 * threshold, 0 = never; with only LM_H2_MAX_ENVS set it is off). */
int lm_step(lm_engine* h, const float* actions, const float* goal_rand, float* out_obs, float* out_states,
            float* out_rew, int64_t* out_resets, float* out_extras, void* stream);

/* Staged form of lm_step for callers that drive the reference's three phases themselves
 * (scripts/random_policy.py:57-61): lm_apply_resets = the reset part of pre_physics_step,
 * lm_substeps(...,1) = one world.step, lm_post_physics = post_physics_step (state read-back,
 * observations, reward, termination; rl_task.py:240-260).  Running apply_resets, controlFrequencyInv
 * sub-steps and post_physics gives the same state as one lm_step. */
int lm_post_physics(lm_engine* h, const float* actions, float* out_obs, float* out_states, float* out_rew,
                    int64_t* out_resets, float* out_extras, void* stream);

/* RLTask.reset(): flag every env for reset (rl_task.py:227-230). */
int lm_reset_all(lm_engine* h, void* stream);

/* Task layer alone on explicit read-back inputs (device float [N][99], layout of oracle LMO_READBACK);
 * uses and updates the handle's task state / counters exactly like the tail of lm_step.
 * Test entry point for the golden vectors captured from the reference's Python. */
int lm_task_eval(lm_engine* h, const float* readback, const float* actions, float* out_obs, float* out_states,
                 float* out_rew, int64_t* out_resets, float* out_extras, void* stream);

/* Only the reset scatter of lm_step (reset_idx, quadruped_pose_control.py:230-299). */
int lm_apply_resets(lm_engine* h, const float* goal_rand, void* stream);

/* n physics sub-steps with given joint-velocity targets (device float [N][12]); no task layer. */
int lm_substeps(lm_engine* h, const float* targets, int n, void* stream);

/* World tip (device float [N][4][3]) and knee ([N][8][3]) positions of the current state. */
int lm_forward_kinematics(lm_engine* h, float* tips, float* knees, void* stream);

/* Debug: dense mass matrix [N][18][18] and bias [N][18] assembled from the limb-aggregate terms. */
int lm_debug_dynamics(lm_engine* h, float* M, float* hvec, void* stream);

void* lm_ptr(lm_engine* h, int kind);
int lm_num_envs(const lm_engine* h);
int lm_num_obs(const lm_engine* h);      /* observation width of this engine (64 or 88) */
int lm_set_seed(lm_engine* h, uint32_t seed);
const char* lm_last_error(void);
const char* lm_version(void);
int lm_abi_version(void);                /* LM_ABI_VERSION the library was built with */

#ifdef __cplusplus
}
#endif
#endif
