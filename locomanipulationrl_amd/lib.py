"""ctypes binding of the C-ABI engine library (include/lm_engine.h) + zero-copy torch views.

The HIP library is the product path; there is no CPU fallback.  Importing this module never
touches the GPU; constructing an :class:`Engine` does, and fails loudly when the shared object or
a HIP device is missing.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Optional, Sequence

import numpy as np

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
_SO = os.environ.get("LM_ENGINE_SO", os.path.join(_CSRC, "liblm_engine.so"))     # override: kernel experiments only

STATE_ROWS, CNT_ROWS, NUM_OBS, NUM_STATES, NUM_ACTIONS, NUM_EXTRAS, TABLE_FLOATS, TERM_ROWS, READBACK = 115, 6, 64, 93, 12, 13, 502, 11, 99
DR_PHYS_ROWS, DR_PHYS_MU = 43, 42       # LM_DR_PHYS_ROWS, LM_DR_PHYS_MU
DR_RESET_CHANNELS, DR_RESET_ROWS = 4, 31      # LM_DR_RESET_CHANNELS, LM_DR_RESET_ROWS
DR_MASS_CHANNELS, DR_MASS_ROWS, NUM_BODIES = 3, 23, 21      # LM_DR_MASS_CHANNELS, LM_DR_MASS_ROWS, LM_NUM_BODIES
DR_ACTUATOR_CHANNELS, DR_ACTUATOR_ROWS = 3, 3      # LM_DR_ACTUATOR_CHANNELS, LM_DR_ACTUATOR_ROWS
CONTACT_ROWS = 16        # LM_CONTACT_ROWS
EPISODE_ROWS = 9         # LM_EPISODE_ROWS (include/lm_policy.h)
# rows of the episode record
EPISODE = dict(running_return=0, running_length=1, episodes=2, sum_return=3, sum_length=4, goal=5, timeout=6, failure=7, last_return=8)
TRAJ_COLS, TRAJ_MAX_ENVS = 64, 256      # LM_TRAJ_COLS, LM_TRAJ_MAX_ENVS (include/lm_policy.h)
REPLAY_ROWS = 32         # LM_REPLAY_ROWS (include/lm_policy.h)
# rows of the replay record (qprev: the first of 12)
REPLAY = dict(rows=0, finished=1, done_at=2, goal=3, row0_err=4, qerr=5, sq_sum=6, tracked=7, early=8, first_succ=9, in_window=10, min_v2=11, ret=12,
              window_return=13, v2_first=14, abs_sum=15, qprev=16)
REPLAY_SATURATED, REPLAY_CMD_ERR = 28, 29      # written by PD plans in targets mode only
REPLAY_CMD_ACTIONS, REPLAY_CMD_TARGETS = 0, 1  # LM_REPLAY_CMD_*
ROW_SE = 90              # R_SE: the swing / extension position targets of variants 1 / 2 (12 rows)
PTR_STATE, PTR_CNT, PTR_OBS_BUF, PTR_STATES_BUF, PTR_REW_BUF, PTR_EXTRAS, PTR_STATS, PTR_TERMS, PTR_DR_CNT, PTR_DR_PHYS, PTR_DR_RESET_STATE, PTR_DR_MASS, PTR_CONTACT, PTR_DR_ACTUATOR = range(14)
PTR_ENV_PARAMS = 14      # LM_PTR_ENV_PARAMS
ENV_PARAM_ROWS = DR_PHYS_ROWS + DR_MASS_ROWS + DR_ACTUATOR_ROWS      # LM_ENV_PARAM_ROWS = 69: the three records one after the other
# the hold table of Engine.enable_env_params() by name: (first row, rows); one row gives a (N,) view, several a (rows, N) one.  The layouts are
# those of dr_phys + dr_mu, dr_mass and dr_actuator; body_masses is in RobotModel.table_body_order()
ENV_PARAMS = dict(max_efforts=(0, 12), max_velocities=(12, 12), gravity=(24, 3), base_force=(27, 3), joint_damping=(30, 12), mu=(DR_PHYS_MU, 1),
                  plate_mass=(DR_PHYS_ROWS, 1), plate_inertia_factor=(DR_PHYS_ROWS + 1, 1), body_masses=(DR_PHYS_ROWS + 2, NUM_BODIES),
                  kp=(DR_PHYS_ROWS + DR_MASS_ROWS, 1), kd=(DR_PHYS_ROWS + DR_MASS_ROWS + 1, 1), latency=(DR_PHYS_ROWS + DR_MASS_ROWS + 2, 1))


def env_param_rows(name: str):
    """(row0, nrows) of a named group of the hold table; ValueError for a name that is none of ENV_PARAMS."""
    if name not in ENV_PARAMS:
        raise ValueError(f"unknown env parameter {name!r}: one of {sorted(ENV_PARAMS)}")
    return ENV_PARAMS[name]


def env_param_shape(name: str, num_envs: int):
    """Shape of the values Engine.set_env_params(name=...) takes: (N,) for a one-row group, (rows, N) otherwise."""
    _, n = env_param_rows(name)
    return (int(num_envs),) if n == 1 else (n, int(num_envs))


def env_param_values(name: str, values, num_envs: int) -> np.ndarray:
    """`values` as the contiguous host float32 (nrows, N) block lm_set_env_params takes; a python scalar holds every env at that value.
    ValueError for an unknown name or a shape other than env_param_shape(name, N)."""
    row0, n = env_param_rows(name)
    if hasattr(values, "detach"):
        values = values.detach().cpu().numpy()
    a = np.asarray(values, dtype=np.float32)
    want = env_param_shape(name, num_envs)
    if a.ndim == 0:
        a = np.full(want, float(a), dtype=np.float32)
    if tuple(a.shape) != want:
        raise ValueError(f"env parameter {name!r}: values of shape {want} are needed (SoA: one row per component, one column per env), got {tuple(a.shape)}")
    return np.ascontiguousarray(a.reshape(n, int(num_envs)))

# names of the exported C symbols (checked by tests/test_abi.py against include/lm_engine.h)
EXPORTS = ["lm_create", "lm_destroy", "lm_set_reset_randomization", "lm_set_mass_randomization", "lm_set_actuator_randomization", "lm_enable_contact_forces", "lm_enable_env_params", "lm_set_env_params", "lm_clear_env_params", "lm_env_params_held", "lm_step", "lm_post_physics", "lm_reset_all", "lm_task_eval", "lm_apply_resets", "lm_substeps",
           "lm_forward_kinematics", "lm_debug_dynamics", "lm_ptr", "lm_num_envs", "lm_num_obs", "lm_set_seed", "lm_last_error", "lm_version", "lm_abi_version",
           "lm_gnn_param_count", "lm_gnn_forward", "lm_mlp_param_count", "lm_mlp_forward", "lm_mlp_param_count_obs", "lm_mlp_forward_obs",
           "lm_sample_actions", "lm_rollout_create", "lm_rollout_run", "lm_rollout_destroy",
           "lm_rollout_set_deterministic", "lm_rollout_set_episode_record", "lm_episode_update",
           "lm_rollout_set_trajectory_record", "lm_trajectory_update",
           "lm_replay_create", "lm_replay_create_pd", "lm_replay_steps", "lm_replay_update", "lm_replay_destroy",
           "lm_mlp_grad_param_count", "lm_mlp_ppo_grad", "lm_mlp_ppo_grad_workspace", "lm_mlp_ppo_grad_geometry", "lm_gae",
           "lm_gnn_grad_param_count", "lm_gnn_ppo_grad", "lm_gnn_ppo_grad_workspace", "lm_gnn_ppo_grad_geometry",
           "lm_optim_state_len", "lm_optim_state_init", "lm_adam_clip_step", "lm_kl_adaptive_lr",
           "lm_mlp_pack_params", "lm_gnn_pack_params", "lm_ppo_batch_sums_len", "lm_ppo_batch_stats_workspace", "lm_ppo_batch_stats", "lm_ppo_batch_apply"]

# rows of the SoA float state
ROW = dict(base_pos=0, base_quat=3, base_lin=7, base_ang=10, q=13, qd=25, plate_pos=37, plate_quat=40, plate_lin=44,
           plate_ang=47, last_actions=50, last_qd=62, last_tip=74, goal=86)
CNT = dict(successes=0, consecutive_successes=1, goal_reset_buf=2, reset_buf=3, progress_buf=4, episode_count=5)


class LmDrChannel(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("operation", C.c_int32), ("distribution", C.c_int32), ("interval", C.c_int32),
                ("p0", C.c_float * 3), ("p1", C.c_float * 3)]


class LmResetDr(C.Structure):
    """lm_reset_dr: the four reset-state channels of one parameter block (joint_positions, joint_velocities, position, orientation)."""
    _fields_ = [("ch", LmDrChannel * DR_RESET_CHANNELS)]


def _fill_channel(dst, ch):
    dst.enabled, dst.operation, dst.distribution, dst.interval = int(ch.enabled), int(ch.operation), int(ch.distribution), int(ch.interval)
    for c in range(3):
        dst.p0[c] = float(ch.p0[c]); dst.p1[c] = float(ch.p1[c])


def _make_dr(struct, ep, attr):
    """The channel list EngineParams.<attr> -> a fresh C struct of a setter family (all channels off for a block that carries none)."""
    r = struct()
    for i, ch in enumerate(getattr(ep, attr, None) or []):
        _fill_channel(r.ch[i], ch)
    return r


def make_reset_dr(ep) -> LmResetDr:
    """EngineParams.dr_reset -> C struct (all channels off for a block that carries none)."""
    return _make_dr(LmResetDr, ep, "dr_reset")


class LmMassDr(C.Structure):
    """lm_mass_dr: the three mass channels of one parameter block (plate mass, plate density, body masses) and the per-body parameters of
    the last one, in table order."""
    _fields_ = [("ch", LmDrChannel * DR_MASS_CHANNELS), ("body_p0", C.c_float * NUM_BODIES), ("body_p1", C.c_float * NUM_BODIES)]


def make_mass_dr(ep) -> LmMassDr:
    """EngineParams.dr_mass / dr_mass_body_p0 / dr_mass_body_p1 -> C struct (all channels off for a block that carries none)."""
    r = _make_dr(LmMassDr, ep, "dr_mass")
    for dst, name in ((r.body_p0, "dr_mass_body_p0"), (r.body_p1, "dr_mass_body_p1")):
        vals = list(getattr(ep, name, None) or [])
        if vals and len(vals) != NUM_BODIES:
            raise ValueError(f"EngineParams.{name}: {NUM_BODIES} values (table order) are needed, got {len(vals)}")
        for k, x in enumerate(vals):
            dst[k] = float(x)
    return r


class LmActuatorDr(C.Structure):
    """lm_actuator_dr: the three actuator channels of one parameter block (kp, kd, command latency)."""
    _fields_ = [("ch", LmDrChannel * DR_ACTUATOR_CHANNELS)]


def make_actuator_dr(ep) -> LmActuatorDr:
    """EngineParams.dr_actuator -> C struct (all channels off for a block that carries none)."""
    return _make_dr(LmActuatorDr, ep, "dr_actuator")


# the setter families of the domain randomisation: EngineParams attribute, maker of the C struct, C entry point
_DR_FAMILIES = (("dr_reset", make_reset_dr, "lm_set_reset_randomization"), ("dr_mass", make_mass_dr, "lm_set_mass_randomization"),
                ("dr_actuator", make_actuator_dr, "lm_set_actuator_randomization"))


class LmPpoHyper(C.Structure):
    """lm_ppo_hyper (include/lm_policy.h): ratio clip, value clip, value-loss scale, entropy scale."""
    _fields_ = [("ratio_clip", C.c_float), ("value_clip", C.c_float), ("value_scale", C.c_float), ("entropy_scale", C.c_float)]


class LmOptimHyper(C.Structure):
    """lm_optim_hyper (include/lm_policy.h): Adam's betas and eps, the gradient-norm clip, the optional floor range."""
    _fields_ = [("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("max_norm", C.c_double),
                ("clamp_offset", C.c_int32), ("clamp_count", C.c_int32), ("clamp_min", C.c_float), ("reserved0", C.c_int32)]


ABI_VERSION = 5          # LM_ABI_VERSION of include/lm_engine.h this mirror was written against


class LmParams(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("params_size", C.c_int32), ("table_floats", C.c_int32), ("reserved0", C.c_int32),
        ("dt", C.c_float), ("kd", C.c_float), ("tau_max", C.c_float), ("act_scale", C.c_float), ("mu", C.c_float),
        ("tip_radius", C.c_float), ("baumgarte", C.c_float), ("max_depen_vel", C.c_float), ("max_joint_vel", C.c_float), ("gravity", C.c_float),
        ("substeps", C.c_int32), ("pgs_iters", C.c_int32), ("mode", C.c_int32),
        ("fixed_base_pos", C.c_float * 3), ("fixed_base_quat", C.c_float * 4),
        ("plate_mass", C.c_float), ("plate_com", C.c_float * 3), ("plate_inertia", C.c_float * 3),
        ("plate_half", C.c_float * 3), ("plate_center", C.c_float * 3),
        ("init_q", C.c_float * 12), ("init_base_pos", C.c_float * 3), ("init_base_quat", C.c_float * 4),
        ("init_plate_pos", C.c_float * 3), ("init_plate_quat", C.c_float * 4),
        ("default_tip", C.c_float * 12), ("goal_lo", C.c_float * 3), ("goal_hi", C.c_float * 3),
        ("s_pos", C.c_float), ("s_lin", C.c_float), ("s_ang", C.c_float), ("s_q", C.c_float), ("s_qd", C.c_float),
        ("quat_scale", C.c_float), ("rot_eps", C.c_float), ("trans_scale", C.c_float), ("acc_scale", C.c_float),
        ("rate_scale", C.c_float), ("bonus", C.c_float), ("limit_pen", C.c_float), ("fall_pen", C.c_float),
        ("succ_thresh", C.c_float),
        ("max_consec", C.c_int32), ("max_episode", C.c_int32),
        ("d23_pen", C.c_float * 2), ("d23_rst", C.c_float * 2), ("d1_pen", (C.c_float * 2) * 4), ("d1_rst", (C.c_float * 2) * 4),
        ("h_base", C.c_float), ("h_corner", C.c_float), ("h_knee", C.c_float), ("corner", (C.c_float * 3) * 4),
        ("clip_obs", C.c_float), ("clip_actions", C.c_float),
        ("max_reset_counts", C.c_int32),
        ("variant", C.c_int32), ("num_obs", C.c_int32), ("pd_kp", C.c_float), ("joint_damping", C.c_float), ("act_scale_se", C.c_float),
        ("se_lo", C.c_float * 12), ("se_hi", C.c_float * 12), ("init_se", C.c_float * 12),
        ("torque_div", C.c_float), ("power_scale", C.c_float), ("target_err_scale", C.c_float), ("rot_dec_scale", C.c_float),
        ("rot_dec_thresh", C.c_float), ("cc_update_last_tgt", C.c_int32), ("acc_substeps", C.c_int32),
        ("dr_enabled", C.c_int32), ("dr_min_frequency", C.c_int32), ("dr", LmDrChannel * 9), ("drive_mode", C.c_int32), ("pd_second_pass", C.c_int32),
        ("dr_mat", LmDrChannel * 2), ("dr_mat_buckets", C.c_int32 * 2), ("mat_mu_robot", C.c_float), ("mat_mu_other", C.c_float),
        ("friction_combine", C.c_int32), ("friction_scale", C.c_float),
        ("plate_si", C.c_float * 10), ("plate_phi", C.c_float * 36), ("ctrl_dt_inv", C.c_float), ("acc_dt_inv", C.c_float),
    ]


_DERIVED = {"plate_si", "plate_phi", "ctrl_dt_inv", "acc_dt_inv", "abi_version", "params_size", "table_floats", "reserved0"}


def make_params(ep, clip_obs: float = 5.0, clip_actions: float = 1.0) -> LmParams:
    """EngineParams -> C struct (clipObservations / clipActions: QuadrupedPoseControl.yaml:11-12)."""
    if getattr(ep, "solver", 0):
        raise ValueError("EngineParams.solver != 0 is an oracle-only experiment (DESIGN.md 2.2): the engine implements solver 0")
    if getattr(ep, "pyramid", 0):
        raise ValueError("EngineParams.pyramid is an oracle-only evidence switch: the engine implements the friction cone only")
    if any(ch.enabled for ch in ep.dr_mat) and abs(ep.material_mu() - ep.mu) > 1e-6 * max(1.0, abs(ep.mu)):
        raise ValueError(f"EngineParams: mu {ep.mu} differs from friction_scale x combine(mat_mu_robot, mat_mu_other) = {ep.material_mu()}: a "
                         "contact-material channel would move the nominal coefficient (set the material fields consistently with mu)")
    p = LmParams()
    p.abi_version, p.params_size, p.table_floats = ABI_VERSION, C.sizeof(LmParams), TABLE_FLOATS      # the stamp lm_create checks
    for name, _ in LmParams._fields_:
        if name in _DERIVED:
            continue
        if name == "clip_obs":
            p.clip_obs = float(clip_obs); continue
        if name == "clip_actions":
            p.clip_actions = float(clip_actions); continue
        if name in ("dr", "dr_mat"):
            dst = getattr(p, name)
            for i, ch in enumerate(getattr(ep, name)):
                _fill_channel(dst[i], ch)
            continue
        if name == "dr_mat_buckets":
            for i, k in enumerate(ep.dr_mat_buckets):
                p.dr_mat_buckets[i] = int(k)
            continue
        val = getattr(ep, name)
        if isinstance(val, (list, tuple, np.ndarray)):
            arr = np.asarray(val, dtype=np.float64)
            dst = getattr(p, name)
            if arr.ndim == 1:
                for i, x in enumerate(arr):
                    dst[i] = float(x)
            else:
                for i, row in enumerate(arr):
                    for j, x in enumerate(row):
                        dst[i][j] = float(x)
        else:
            setattr(p, name, val)
    return p


def hipcc_command(extra, out):
    """The ONE hipcc command line of the engine: the product build and every diagnostic build (tools/stamp_profile*.py, tools/ab_build.py: `extra` =
    their -D switches) compile with the same flags, so that a diagnostic library measures the product's code."""
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    # -fno-slp-vectorize: the SLP vectoriser's own packed-fp32 pairs cost more v_mov / AGPR shuffles than they save (round 1: 56.0 -> 58.2 M
    #   env-steps/s without it); the packed fp32 the kernel relies on is written by hand on the f2 type (lm_math.h) and is not affected
    # -fno-hip-fp32-correctly-rounded-divide-sqrt: 1/x and sqrt as v_rcp / v_sqrt (1 ulp) instead of the ~10-instruction IEEE sequences
    # -amdgpu-mfma-vgpr-form: the MFMA accumulators of the policy tiles live in ordinary VGPRs, so the VALU work on them (ELU, max aggregation,
    # LDS stores) needs no v_accvgpr_read per element (504 of them in k_gnn_forward)
    return [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-fno-hip-fp32-correctly-rounded-divide-sqrt",
            "-mllvm", "-amdgpu-mfma-vgpr-form", "-fPIC", "-shared", *extra, os.path.join(_CSRC, "lm_engine.hip"), os.path.join(_CSRC, "lm_engine_w2.hip"), os.path.join(_CSRC, "lm_engine_h2.hip"), os.path.join(_CSRC, "lm_engine_h3.hip"), os.path.join(_CSRC, "lm_engine_ev.hip"), os.path.join(_CSRC, "lm_engine_tr.hip"), os.path.join(_CSRC, "lm_engine_hp.hip"),
            os.path.join(_CSRC, "lm_policy.hip"), os.path.join(_CSRC, "lm_ppo.hip"), os.path.join(_CSRC, "lm_gnn_ppo.hip"), os.path.join(_CSRC, "lm_optim.hip"), os.path.join(_CSRC, "lm_prepare.hip"), os.path.join(_CSRC, "lm_replay.hip"), "-o", out]


def build_library(force: bool = False, verbose: bool = False) -> str:
    """Compile the engine (csrc/*.hip) for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    inc = os.path.join(os.path.dirname(os.path.dirname(_CSRC)), "include")
    import glob
    deps = sorted(glob.glob(os.path.join(_CSRC, "*.hip")) + glob.glob(os.path.join(_CSRC, "*.h")) + glob.glob(os.path.join(inc, "*.h")))      # every source the .so is built from
    if not force and os.path.exists(_SO) and all(os.path.getmtime(_SO) >= os.path.getmtime(d) for d in deps):
        return _SO
    cmd = hipcc_command(extra=[], out=_SO)
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return _SO


_lib = None


def load_library() -> C.CDLL:
    """dlopen the engine; raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise RuntimeError(f"{_SO} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(the engine has no CPU fallback)")
    lib = C.CDLL(_SO)
    vp, fp, ip = C.c_void_p, C.c_void_p, C.c_int
    lib.lm_create.argtypes = [C.POINTER(vp), ip, C.c_void_p, C.POINTER(LmParams), ip, ip, C.c_uint32]
    lib.lm_destroy.argtypes = [vp]
    lib.lm_set_reset_randomization.argtypes = [vp, ip, C.POINTER(LmResetDr)]
    lib.lm_set_mass_randomization.argtypes = [vp, ip, C.POINTER(LmMassDr)]
    lib.lm_set_actuator_randomization.argtypes = [vp, ip, C.POINTER(LmActuatorDr)]
    lib.lm_enable_contact_forces.argtypes = [vp, ip]
    lib.lm_enable_env_params.argtypes = [vp]
    lib.lm_set_env_params.argtypes = [vp, ip, ip, fp]
    lib.lm_clear_env_params.argtypes = [vp, ip, ip]
    lib.lm_env_params_held.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.lm_step.argtypes = [vp, fp, fp, fp, fp, fp, fp, fp, vp]
    lib.lm_post_physics.argtypes = [vp, fp, fp, fp, fp, fp, fp, vp]
    lib.lm_reset_all.argtypes = [vp, vp]
    lib.lm_task_eval.argtypes = [vp, fp, fp, fp, fp, fp, fp, fp, vp]
    lib.lm_apply_resets.argtypes = [vp, fp, vp]
    lib.lm_substeps.argtypes = [vp, fp, ip, vp]
    lib.lm_forward_kinematics.argtypes = [vp, fp, fp, vp]
    lib.lm_debug_dynamics.argtypes = [vp, fp, fp, vp]
    lib.lm_ptr.argtypes = [vp, ip]; lib.lm_ptr.restype = vp
    lib.lm_num_envs.argtypes = [vp]
    lib.lm_num_obs.argtypes = [vp]
    lib.lm_set_seed.argtypes = [vp, C.c_uint32]
    lib.lm_internal_step_variant.argtypes = [vp]      # not part of the C ABI (include/lm_engine.h): which step kernel an engine runs
    lib.lm_gnn_forward.argtypes = [fp, ip, fp, fp, fp, vp]
    lib.lm_mlp_forward.argtypes = [fp, ip, fp, fp, fp, vp]
    lib.lm_mlp_param_count_obs.argtypes = [ip]
    lib.lm_mlp_forward_obs.argtypes = [fp, ip, ip, fp, fp, fp, vp]
    lib.lm_sample_actions.argtypes = [fp, fp, vp, ip, C.c_uint32, fp, fp, vp]
    lib.lm_rollout_create.argtypes = [C.POINTER(vp), vp, ip, fp, fp, ip, C.c_uint32, fp, fp, fp, fp, fp, vp, fp]
    lib.lm_rollout_run.argtypes = [vp, ip, vp]
    lib.lm_rollout_destroy.argtypes = [vp]
    lib.lm_rollout_set_deterministic.argtypes = [vp, ip]
    lib.lm_rollout_set_episode_record.argtypes = [vp, fp, ip]
    lib.lm_episode_update.argtypes = [vp, fp, vp, fp, ip, vp]
    lib.lm_rollout_set_trajectory_record.argtypes = [vp, vp, ip, fp, vp, ip, ip]
    lib.lm_trajectory_update.argtypes = [vp, vp, ip, fp, vp, fp, vp, ip, ip, vp]
    lib.lm_replay_create.argtypes = [C.POINTER(vp), vp, fp, fp, vp, ip, ip, vp, ip, ip, ip, C.c_float, C.c_float, C.c_float]
    lib.lm_replay_create_pd.argtypes = [C.POINTER(vp), vp, fp, fp, vp, ip, ip, vp, ip, ip, ip, C.c_float, C.c_float]
    lib.lm_replay_steps.argtypes = [vp]
    lib.lm_replay_update.argtypes = [vp, ip, fp, fp, fp, fp, vp]
    lib.lm_replay_destroy.argtypes = [vp]
    lib.lm_mlp_grad_param_count.argtypes = [ip]
    lib.lm_mlp_ppo_grad.argtypes = [fp, fp, fp, fp, fp, fp, fp, ip, ip, C.POINTER(LmPpoHyper), fp, fp, vp, C.c_longlong, vp]
    lib.lm_mlp_ppo_grad_workspace.argtypes = [ip, ip]; lib.lm_mlp_ppo_grad_workspace.restype = C.c_longlong
    lib.lm_mlp_ppo_grad_geometry.argtypes = [ip, ip, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.lm_gae.argtypes = [fp, fp, vp, fp, ip, ip, C.c_double, C.c_double, fp, fp, vp]
    lib.lm_gnn_ppo_grad.argtypes = [fp, fp, fp, fp, fp, fp, fp, ip, C.POINTER(LmPpoHyper), fp, fp, vp, C.c_longlong, vp]
    lib.lm_gnn_ppo_grad_workspace.argtypes = [ip]; lib.lm_gnn_ppo_grad_workspace.restype = C.c_longlong
    lib.lm_gnn_ppo_grad_geometry.argtypes = [ip, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.lm_optim_state_init.argtypes = [fp, C.c_double, C.c_double, vp]
    lib.lm_adam_clip_step.argtypes = [fp, fp, fp, fp, ip, fp, C.POINTER(LmOptimHyper), vp]
    lib.lm_kl_adaptive_lr.argtypes = [fp, fp, ip, C.c_double, C.c_double, C.c_double, vp]
    lib.lm_mlp_pack_params.argtypes = [fp, ip, fp, C.c_double, C.c_double, fp, vp, vp]
    lib.lm_gnn_pack_params.argtypes = [fp, ip, fp, C.c_double, C.c_double, fp, vp, vp]
    lib.lm_ppo_batch_sums_len.argtypes = [ip]
    lib.lm_ppo_batch_stats_workspace.argtypes = [ip, ip]; lib.lm_ppo_batch_stats_workspace.restype = C.c_longlong
    lib.lm_ppo_batch_stats.argtypes = [fp, fp, fp, ip, ip, fp, vp, C.c_longlong, vp]
    lib.lm_ppo_batch_apply.argtypes = [fp, fp, fp, fp, ip, ip, fp, fp, fp, ip, C.c_double, C.c_double, fp, fp, fp, fp, vp]
    lib.lm_last_error.restype = C.c_char_p
    lib.lm_version.restype = C.c_char_p
    _lib = lib
    return lib


class EngineError(RuntimeError):
    pass


class _DevArray:
    """Minimal __cuda_array_interface__ carrier so torch can wrap handle-owned device memory zero-copy."""

    def __init__(self, ptr: int, shape, typestr: str, owner):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}
        self._owner = owner


class Engine:
    """One engine instance = N lock-step environments on one GPU (one process per GPU)."""

    def __init__(self, robot_model, params: Sequence, num_envs: int, split_env: Optional[int] = None, seed: int = 42,
                 device: str = "cuda:0", clip_obs: float = 5.0, clip_actions: float = 1.0):
        import torch
        if not torch.cuda.is_available():
            raise EngineError("no HIP device visible: the engine runs on MI355X only (no CPU fallback)")
        self.torch = torch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise EngineError(f"the engine runs on a HIP device, not {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lib = load_library()
        self.num_envs = int(num_envs)
        params = list(params)
        arr = (LmParams * len(params))(*[make_params(p, clip_obs, clip_actions) for p in params])
        table = np.ascontiguousarray(robot_model.packed_table(), dtype=np.float32)
        assert table.shape == (TABLE_FLOATS,)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = self.lib.lm_create(C.byref(self._h), self.num_envs, table.ctypes.data_as(C.c_void_p), arr, len(params),
                                    int(split_env or 0), C.c_uint32(seed))
        self._check(rc)
        for b, ep in enumerate(params):          # reset-state, mass and actuator channels: handed over per block, before the first step
            for attr, make, setter in _DR_FAMILIES:
                if any(ch.enabled for ch in (getattr(ep, attr, None) or [])):
                    dr = make(ep)
                    with torch.cuda.device(self.device):
                        self._check(getattr(self.lib, setter)(self._h, b, C.byref(dr)))
        self.seed = int(seed) & 0xFFFFFFFF
        self.params = params                     # the parameter blocks as handed in (host side: what a ReplayPlan reads act_scale and the control period from)
        self.split_env = int(split_env) if (split_env and len(params) == 2) else None      # first env of the second parameter block (co-training)
        N = self.num_envs
        self.state = self._wrap(PTR_STATE, (STATE_ROWS, N), "<f4")
        self.cnt = self._wrap(PTR_CNT, (CNT_ROWS, N), "<i8")
        self.num_obs = int(self.lib.lm_num_obs(self._h))
        self._views = {}            # obs_buf / states_buf / terms: asked for on first access (lm_step writes them only from then on)
        self._steps_run = 0         # lm_step calls so far (a first view request after stepping is stale: warned about)
        self.rew_buf = self._wrap(PTR_REW_BUF, (N,), "<f4")
        self.extras_buf = self._wrap(PTR_EXTRAS, (NUM_EXTRAS,), "<f4")
        self.stats_i64 = self._wrap(PTR_STATS, (6,), "<i8")
        self._stats_i32 = self._wrap(PTR_STATS, (16,), "<i4")         # word 15: contained blow-ups
        self.dr_cnt = self._wrap(PTR_DR_CNT, (5, N), "<i8")          # domain-randomisation counters
        self.dr_phys = self._wrap(PTR_DR_PHYS, (42, N), "<f4")       # attributes sampled for the last step (rows 0..41)
        self.dr_mu = self._wrap(PTR_DR_PHYS, (DR_PHYS_ROWS, N), "<f4")[DR_PHYS_MU]      # row 42: the contact mu of each env in the last step

    def _view(self, kind, shape):
        if kind not in self._views:
            if self._steps_run:
                # lm_step starts writing this buffer with the NEXT step: what it holds now is zeros or an older step's values
                import warnings
                warnings.warn("lm_engine: an unclipped view (obs_buf / states_buf / terms) was first requested after %d step(s): it is stale until the next "
                              "step (ask for it before stepping; include/lm_engine.h, lm_ptr_kind)" % self._steps_run, RuntimeWarning, stacklevel=3)
            self._views[kind] = self._wrap(kind, shape, "<f4")
        return self._views[kind]

    # The engine's own unclipped copies of what step() hands out clipped (task.obs_buf / states_buf of rl_task.py:104-113, the per-env reward
    # terms).  lm_step keeps one current only after its pointer has been asked for (lm_ptr), or when step() is called without the matching
    # output tensor: a caller that consumes out_obs / out_states alone does not pay for the second copy (672 B per env-step of stores).
    @property
    def obs_buf(self):
        return self._view(PTR_OBS_BUF, (self.num_envs, self.num_obs))

    @property
    def states_buf(self):
        return self._view(PTR_STATES_BUF, (self.num_envs, NUM_STATES))

    @property
    def terms(self):
        return self._view(PTR_TERMS, (TERM_ROWS, self.num_envs))

    def _record(self, name, kind, rows, missing):
        """float [rows][N] view of a record that exists only on engines that asked for it (lm_ptr gives NULL otherwise: EngineError(missing))."""
        if name not in self._views:
            ptr = self.lib.lm_ptr(self._h, kind)
            if not ptr:
                raise EngineError(missing)
            self._views[name] = self.torch.as_tensor(_DevArray(ptr, (rows, self.num_envs), "<f4", self), device=self.device)
        return self._views[name]

    @property
    def dr_reset_state(self):
        """float [31][N]: the state each env was last reset to by step() - q 12, qd 12, free-body position 3, quaternion (w, x, y, z) 4 -
        nominal resets included.  Randomised engines only (dr_enabled)."""
        return self._record("dr_reset_state", PTR_DR_RESET_STATE, DR_RESET_ROWS, "dr_reset_state: the engine was created without dr_enabled (no reset-state record)")

    @property
    def dr_mass(self):
        """float [23][N]: the masses the last step used, floored - row 0 the plate's mass, row 1 the factor on its inertia about the COM,
        rows 2..22 the 21 body masses in table order (RobotModel.table_body_order()).  The nominal values until a mass channel draws.
        Randomised engines only (dr_enabled)."""
        return self._record("dr_mass", PTR_DR_MASS, DR_MASS_ROWS, "dr_mass: the engine was created without dr_enabled (no mass record)")

    @property
    def dr_plate_mass(self):
        """float [N]: row 0 of dr_mass."""
        return self.dr_mass[0]

    @property
    def dr_body_masses(self):
        """float [21][N]: rows 2..22 of dr_mass (table order)."""
        return self.dr_mass[2:]

    # ------------------------------------------------------------------ contact-force reporting
    def enable_contact_forces(self, on: bool = True):
        """Switch per-foot contact-force reporting on (or off again): step() and substeps() then also write the contact record, from
        reporting builds of their kernels; an engine that never asks runs the kernels it always ran.  The record is a derived output
        of the last step, not part of state_dict()."""
        with self.torch.cuda.device(self.device):
            self._check(self.lib.lm_enable_contact_forces(self._h, 1 if on else 0))

    def _contact_record(self):
        return self._record("contact", PTR_CONTACT, CONTACT_ROWS, "contact forces are not reported by this engine: call enable_contact_forces() first "
                            "(task YAML: sim.engine.contact_forces: true)")

    @property
    def contact_forces(self):
        """float (N, 4, 3), a zero-copy view of the record's SoA rows: the force on each foot (limb order of the state) by the ground /
        the plate, world frame, newtons, averaged over the sub-steps of the last step() or substeps() call."""
        return self._contact_record()[:12].T.reshape(self.num_envs, 4, 3)

    @property
    def contact_fraction(self):
        """float (N, 4) view: the share of the last step's sub-steps in which each foot was loaded (lam_n > 0), a multiple of 1 / n_sub."""
        return self._contact_record()[12:16].T

    # ------------------------------------------------------------------ per-env parameters held by the caller
    def enable_env_params(self):
        """Allocate the hold table (nothing held): from now on step() launches the builds of the randomised kernels that apply held rows.
        Randomised engines only (dr_enabled, with or without channels); not together with contact-force reporting."""
        with self.torch.cuda.device(self.device):
            self._check(self.lib.lm_enable_env_params(self._h))

    @property
    def env_params_enabled(self) -> bool:
        return bool(self.lib.lm_ptr(self._h, PTR_ENV_PARAMS))

    def _env_table(self):
        return self._record("env_params", PTR_ENV_PARAMS, ENV_PARAM_ROWS, "env params are not enabled on this engine: call enable_env_params() first "
                            "(task YAML: sim.engine.env_params: true)")

    def set_env_params(self, **named):
        """Hold the named groups (ENV_PARAMS) at per-env values: SoA arrays / tensors of env_param_shape(name, N), or a scalar for every env.
        Every later step uses them in place of what the group's channel draws (or of the nominal value); the dr_* records report them.
        The call waits for the device first: a step enqueued before it, on any stream, still runs with the rows as they were.
        Validated by the library (EngineError, nothing changed) - finite; masses, plate_inertia_factor, kp, kd > 0; mu, max_efforts,
        max_velocities, joint_damping >= 0; latency whole in [0, substeps]; groups the engine's blocks do not read are refused.  Names and
        shapes of all groups are checked first (ValueError); each group is then one library call, so the groups in front of a refused one
        stay held."""
        blocks = [(env_param_rows(k)[0], env_param_values(k, v, self.num_envs)) for k, v in named.items()]      # every name and shape first
        self._env_table()
        with self.torch.cuda.device(self.device):
            for row0, a in blocks:
                self._check(self.lib.lm_set_env_params(self._h, row0, a.shape[0], a.ctypes.data_as(C.c_void_p)))

    def clear_env_params(self, *names):
        """The named groups follow their channel (or the nominal value) again from the next step on; without names, all of them.  Waits for
        the device first, as set_env_params does: steps enqueued before the call still run with the rows held."""
        spans = [env_param_rows(k) for k in names] or [(0, ENV_PARAM_ROWS)]
        self._env_table()
        with self.torch.cuda.device(self.device):
            for row0, n in spans:
                self._check(self.lib.lm_clear_env_params(self._h, row0, n))

    def env_params_mask(self):
        """bool (69,) numpy array: which rows of the hold table are held."""
        m = (C.c_uint64 * 2)()
        self._check(self.lib.lm_env_params_held(self._h, m))
        return np.array([(int(m[r >> 6]) >> (r & 63)) & 1 for r in range(ENV_PARAM_ROWS)], dtype=bool)

    @property
    def env_params_held(self):
        """Names of the groups that are held (every row of the group)."""
        m = self.env_params_mask()
        return [k for k, (r0, n) in ENV_PARAMS.items() if m[r0:r0 + n].all()]

    @property
    def env_params(self):
        """dict name -> zero-copy view of the hold table ((N,) or (rows, N), ENV_PARAMS).  Rows that are not held read as what was last held
        there (zeros at first); change values through set_env_params, which validates them."""
        t = self._env_table()
        return {k: (t[r0] if n == 1 else t[r0:r0 + n]) for k, (r0, n) in ENV_PARAMS.items()}

    @property
    def dr_actuator(self):
        """float [3][N]: what the last step used - row 0 the position gain kp, row 1 the velocity gain kd (both floored), row 2 the command
        latency d in sub-steps.  The nominal values (pd_kp, kd, 0) until an actuator channel draws.  Randomised engines only (dr_enabled)."""
        return self._record("dr_actuator", PTR_DR_ACTUATOR, DR_ACTUATOR_ROWS, "dr_actuator: the engine was created without dr_enabled (no actuator record)")

    @property
    def dr_kp(self):
        """float [N]: row 0 of dr_actuator."""
        return self.dr_actuator[0]

    @property
    def dr_kd(self):
        """float [N]: row 1 of dr_actuator."""
        return self.dr_actuator[1]

    @property
    def dr_latency(self):
        """float [N]: row 2 of dr_actuator (whole sub-steps)."""
        return self.dr_actuator[2]

    @property
    def blowups(self) -> int:
        """Envs whose state became non-finite or exploded and was replaced by the reset pose (contained by the kernel's guard)."""
        return int(self._stats_i32[15].item()) & 0xFFFFFFFF

    @property
    def step_variant(self) -> str:
        """The velocity-drive kernel step() launches on this engine: "w1" (k_step, one wavefront per 16 envs), "w2" (k_step_w2, two such workgroups
        per SIMD), "h2" (k_step_h2, a helper wavefront per workgroup) or "h3" (k_step_h3, two helper wavefronts per workgroup); DESIGN.md 5.1.
        Every other kernel family reports "w1"."""
        return ("w1", "w2", "h2", "h3")[self.lib.lm_internal_step_variant(self._h)]

    # ------------------------------------------------------------------
    def _check(self, rc: int):
        if rc != 0:
            raise EngineError(f"lm_engine error {rc}: {self.lib.lm_last_error().decode()}")

    def _wrap(self, kind: int, shape, typestr: str):
        ptr = self.lib.lm_ptr(self._h, kind)
        if not ptr:
            raise EngineError("lm_ptr returned NULL")
        return self.torch.as_tensor(_DevArray(ptr, shape, typestr, self), device=self.device)

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    @staticmethod
    def _p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def _f32(self, t, shape):
        assert t.device == self.device and t.dtype == self.torch.float32 and t.is_contiguous() and tuple(t.shape) == tuple(shape), \
            (t.device, self.device, t.dtype, tuple(t.shape), shape)
        return t

    # ------------------------------------------------------------------ C-ABI calls
    def step(self, actions, goal_rand=None, out_obs=None, out_states=None, out_rew=None, out_resets=None, out_extras=None):
        N = self.num_envs
        self._f32(actions, (N, NUM_ACTIONS))
        if goal_rand is not None:
            self._f32(goal_rand, (N, 3))
        if out_obs is not None: self._f32(out_obs, (N, self.num_obs))
        if out_states is not None: self._f32(out_states, (N, NUM_STATES))
        if out_rew is not None: self._f32(out_rew, (N,))
        if out_extras is not None: self._f32(out_extras, (NUM_EXTRAS,))
        if out_resets is not None:
            assert out_resets.dtype == self.torch.int64 and tuple(out_resets.shape) == (N,) and out_resets.device == self.device and out_resets.is_contiguous()
        self._check(self.lib.lm_step(self._h, self._p(actions), self._p(goal_rand), self._p(out_obs), self._p(out_states),
                                     self._p(out_rew), self._p(out_resets), self._p(out_extras), self._stream()))
        self._steps_run += 1

    def post_physics(self, actions, out_obs=None, out_states=None, out_rew=None, out_resets=None, out_extras=None):
        self._f32(actions, (self.num_envs, NUM_ACTIONS))
        self._check(self.lib.lm_post_physics(self._h, self._p(actions), self._p(out_obs), self._p(out_states), self._p(out_rew),
                                             self._p(out_resets), self._p(out_extras), self._stream()))

    def task_eval(self, readback, actions, out_obs=None, out_states=None, out_rew=None, out_resets=None, out_extras=None):
        N = self.num_envs
        self._f32(readback, (N, READBACK)); self._f32(actions, (N, NUM_ACTIONS))
        self._check(self.lib.lm_task_eval(self._h, self._p(readback), self._p(actions), self._p(out_obs), self._p(out_states),
                                          self._p(out_rew), self._p(out_resets), self._p(out_extras), self._stream()))

    def reset_all(self):
        self._check(self.lib.lm_reset_all(self._h, self._stream()))

    def apply_resets(self, goal_rand=None):
        if goal_rand is not None:
            self._f32(goal_rand, (self.num_envs, 3))
        self._check(self.lib.lm_apply_resets(self._h, self._p(goal_rand), self._stream()))

    def substeps(self, targets, n: int = 1):
        self._f32(targets, (self.num_envs, NUM_ACTIONS))
        self._check(self.lib.lm_substeps(self._h, self._p(targets), int(n), self._stream()))

    def forward_kinematics(self):
        N = self.num_envs
        tips = self.torch.empty((N, 4, 3), dtype=self.torch.float32, device=self.device)
        knees = self.torch.empty((N, 8, 3), dtype=self.torch.float32, device=self.device)
        self._check(self.lib.lm_forward_kinematics(self._h, self._p(tips), self._p(knees), self._stream()))
        return tips, knees

    def debug_dynamics(self):
        N = self.num_envs
        M = self.torch.zeros((N, 18, 18), dtype=self.torch.float32, device=self.device)
        h = self.torch.zeros((N, 18), dtype=self.torch.float32, device=self.device)
        self._check(self.lib.lm_debug_dynamics(self._h, self._p(M), self._p(h), self._stream()))
        return M, h

    def set_seed(self, seed: int):
        self._check(self.lib.lm_set_seed(self._h, C.c_uint32(seed)))
        self.seed = int(seed) & 0xFFFFFFFF

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.torch.cuda.synchronize(self.device)
            self.lib.lm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ convenience (tests / tooling)
    def set_phys_env_major(self, phys):
        """phys: (N,50) env-major array in the oracle's LMO_PHYS layout -> rows 0..49 of the SoA state."""
        t = self.torch.as_tensor(np.ascontiguousarray(phys, dtype=np.float32).T.copy(), device=self.device)
        self.state[:50].copy_(t)

    def get_phys_env_major(self):
        return self.state[:50].T.contiguous().cpu().numpy()

    def set_task_env_major(self, task):
        t = self.torch.as_tensor(np.ascontiguousarray(task, dtype=np.float32).T.copy(), device=self.device)
        self.state[50:50 + t.shape[0]].copy_(t)

    def get_task_env_major(self):
        return self.state[50:115].T.contiguous().cpu().numpy()

    def set_cnt_env_major(self, cnt):
        self.cnt.copy_(self.torch.as_tensor(np.ascontiguousarray(cnt, dtype=np.int64).T.copy(), device=self.device))

    def get_cnt_env_major(self):
        return self.cnt.T.contiguous().cpu().numpy()

    # ------------------------------------------------------------------ simulator checkpoint (the reference never
    # checkpoints simulator state; with a deterministic engine a snapshot + the same actions reproduces a run bit for bit)
    def state_dict(self):
        """Everything lm_step reads besides its arguments: SoA state, counters, success windows, randomisation counters (host tensors)."""
        self.torch.cuda.synchronize(self.device)
        sd = {"state": self.state.cpu().clone(), "cnt": self.cnt.cpu().clone(), "stats": self._stats_i32.cpu().clone(),
              "dr_cnt": self.dr_cnt.cpu().clone(), "num_envs": self.num_envs, "seed": self.seed}
        if self.env_params_enabled:          # the hold table and which of its rows are held (absent on engines that never enabled it)
            sd["env_params"] = {"table": self._env_table().cpu().clone(), "mask": self.torch.from_numpy(self.env_params_mask())}
        return sd

    def load_state_dict(self, sd):
        assert int(sd["num_envs"]) == self.num_envs and tuple(sd["state"].shape) == tuple(self.state.shape)
        self.state.copy_(sd["state"].to(self.device)); self.cnt.copy_(sd["cnt"].to(self.device))
        self._stats_i32.copy_(sd["stats"].to(self.device)); self.dr_cnt.copy_(sd["dr_cnt"].to(self.device))
        if "seed" in sd:          # goal sampling / domain randomisation are keyed by the seed: a resumed engine must carry the checkpoint's
            self.set_seed(int(sd["seed"]))
        if "env_params" in sd:    # held rows go through the validating setter, in runs of adjacent rows; the others are cleared
            self.enable_env_params()
            table = np.ascontiguousarray(sd["env_params"]["table"].cpu().numpy(), dtype=np.float32); mask = np.asarray(sd["env_params"]["mask"].cpu().numpy(), dtype=bool)
            assert table.shape == (ENV_PARAM_ROWS, self.num_envs) and mask.shape == (ENV_PARAM_ROWS,)
            with self.torch.cuda.device(self.device):
                self._check(self.lib.lm_clear_env_params(self._h, 0, ENV_PARAM_ROWS))
                r = 0
                while r < ENV_PARAM_ROWS:
                    if not mask[r]:
                        r += 1; continue
                    r1 = r
                    while r1 < ENV_PARAM_ROWS and mask[r1]:
                        r1 += 1
                    self._check(self.lib.lm_set_env_params(self._h, r, r1 - r, table[r:r1].ctypes.data_as(C.c_void_p)))
                    r = r1


POLICY_MLP, POLICY_GNN = 0, 1


class Rollout:
    """T steps of  policy forward (MFMA) -> gaussian sampling -> lm_step  recorded into rollout buffers and replayed as one hipGraph
    (include/lm_policy.h).  `packed_params` / `log_std` are device tensors read at run time: refresh them in place
    between runs.  Buffers: obs (T+1,N,64) with obs[0] = current observations, actions (T,N,12), logp (T,N), values (T+1,N),
    rewards (T,N), dones int64 (T,N), extras (T,13).

    Evaluation switches (both off by default; a plan that uses neither runs the kernels it always ran): `deterministic` makes actions[t] the
    forward's mean and logp[t] the density at the mean; `episode_record` (an EpisodeRecord or a float (9, N) device tensor) is updated after
    every step, for the first `episode_cap` episodes of each env when the cap is positive; `trajectory_record` (a TrajectoryRecord) gets one
    row per step of its tracked envs, in every mode ("persistent" on the MLP with 64-wide observations; elsewhere it refuses such a plan and
    "auto" takes the graph)."""

    def __init__(self, engine: Engine, policy: int, packed_params, log_std, T: int, noise_seed: int = 0, deterministic: bool = False,
                 episode_record=None, episode_cap: int = 0, trajectory_record=None):
        torch = engine.torch
        self.engine, self.T, self.N = engine, int(T), engine.num_envs
        assert engine.num_obs == 64 or (engine.num_obs == 88 and policy == POLICY_MLP), "the GNN reads the 64-wide layout; the MLP 64 or 88"
        dev = engine.device
        assert packed_params.is_cuda and packed_params.dtype == torch.float32 and packed_params.is_contiguous()
        assert log_std.is_cuda and log_std.dtype == torch.float32 and log_std.numel() == 12 and log_std.is_contiguous()
        n_expected = engine.lib.lm_mlp_param_count_obs(engine.num_obs) if policy == POLICY_MLP else engine.lib.lm_gnn_param_count()
        assert packed_params.numel() == n_expected, (packed_params.numel(), n_expected)
        self.params, self.log_std = packed_params, log_std
        z = lambda *s, dt=torch.float32: torch.zeros(*s, device=dev, dtype=dt)
        T, N = self.T, self.N
        self.obs, self.actions, self.logp, self.values = z(T + 1, N, engine.num_obs), z(T, N, 12), z(T, N), z(T + 1, N)
        self.rewards, self.dones, self.extras = z(T, N), z(T, N, dt=torch.int64), z(T, NUM_EXTRAS)
        self._h = C.c_void_p()
        p = Engine._p
        rc = engine.lib.lm_rollout_create(C.byref(self._h), engine._h, int(policy), p(self.params), p(self.log_std), T, C.c_uint32(noise_seed),
                                          p(self.obs), p(self.actions), p(self.logp), p(self.values), p(self.rewards), p(self.dones), p(self.extras))
        if rc != 0:
            raise EngineError(f"lm_rollout_create failed ({rc})")
        self.deterministic, self.episode_record, self.episode_cap, self.trajectory_record = False, None, 0, None
        if deterministic:
            self.set_deterministic(True)
        if episode_record is not None:
            self.set_episode_record(episode_record, episode_cap)
        if trajectory_record is not None:
            self.set_trajectory_record(trajectory_record)

    def _set(self, rc):
        if rc != 0:
            raise EngineError(f"lm_engine error {rc}: {self.engine.lib.lm_last_error().decode()}")

    def set_deterministic(self, on: bool = True):
        """Mean actions from the next run on (a captured graph is re-captured)."""
        with self.engine.torch.cuda.device(self.engine.device):
            self._set(self.engine.lib.lm_rollout_set_deterministic(self._h, 1 if on else 0))
        self.deterministic = bool(on)

    def set_episode_record(self, record=None, episode_cap: int = 0):
        """Attach an EpisodeRecord / a float (9, N) device tensor (None: recording off) from the next run on; the plan keeps it alive."""
        t = getattr(record, "record", record)
        if t is not None:
            self.engine._f32(t, (EPISODE_ROWS, self.N))
        with self.engine.torch.cuda.device(self.engine.device):
            self._set(self.engine.lib.lm_rollout_set_episode_record(self._h, Engine._p(t), int(episode_cap)))
        self.episode_record, self.episode_cap = record, int(episode_cap)

    def set_trajectory_record(self, record=None):
        """Attach a TrajectoryRecord of this plan's engine (None: recording off) from the next run on; the plan keeps it alive.  Synchronous:
        the env ids are copied to the device before the call returns."""
        lib = self.engine.lib
        with self.engine.torch.cuda.device(self.engine.device):
            if record is None:
                self._set(lib.lm_rollout_set_trajectory_record(self._h, None, 0, None, None, 0, 0))
            else:
                assert record.engine is self.engine, "the record tracks envs of another engine"
                ids = (C.c_int32 * record.K)(*record.env_ids)
                self._set(lib.lm_rollout_set_trajectory_record(self._h, ids, record.K, Engine._p(record.rows), Engine._p(record.header), record.max_rows,
                                                               record.episode_cap))
        self.trajectory_record = record

    MODES = {"enqueue": 0, "graph": 1, "persistent": 2, "auto": 3}

    def run(self, use_graph=True):
        """use_graph: False / "enqueue" (2T+1 launches), True / "graph" (one hipGraph replay) or "persistent" (the whole rollout in one kernel:
        un-randomised engines; pays up to 16 envs x compute units = 4096 envs on MI355X) or "auto" (persistent where it pays, else the graph);
        identical buffers in all modes."""
        mode = self.MODES[use_graph] if isinstance(use_graph, str) else (1 if use_graph else 0)
        rc = self.engine.lib.lm_rollout_run(self._h, mode, self.engine._stream())
        if rc != 0:
            raise EngineError(f"lm_rollout_run failed ({rc}): {self.engine.lib.lm_last_error().decode()}")

    def close(self):
        if self._h:
            self.engine.lib.lm_rollout_destroy(self._h); self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sample_actions(engine: Engine, mean, log_std, seed: int):
    """lm_sample_actions: (actions, logp) for the engine's current counters."""
    torch = engine.torch
    N = engine.num_envs
    act = torch.empty((N, 12), device=engine.device); logp = torch.empty((N,), device=engine.device)
    p = Engine._p
    rc = engine.lib.lm_sample_actions(p(mean.contiguous()), p(log_std.contiguous()), p(engine.cnt), N, C.c_uint32(seed), p(act), p(logp), engine._stream())
    if rc != 0:
        raise EngineError(f"lm_sample_actions failed ({rc})")
    return act, logp


class EpisodeRecord:
    """The episode record of include/lm_policy.h: a float (9, N) tensor on the engine's device - per env the running return and length, the
    episodes completed, the sums of their returns and lengths, how they ended (goal / timeout / failure) and the last return (rows: EPISODE).
    Hand it to a Rollout (episode_record=) or call update() after every engine step; zero() starts a measurement.  On an engine without
    the C library (CPU tensors: the oracle backend of the tests) update() applies the same rule in torch."""

    def __init__(self, engine):
        import torch
        self.torch, self.engine, self.N = torch, engine, int(engine.num_envs)
        self.record = torch.zeros((EPISODE_ROWS, self.N), dtype=torch.float32, device=engine.cnt.device)
        self._native = hasattr(engine, "lib") and hasattr(engine, "_h")
        if self._native:
            self.split = engine.split_env
        else:                     # a backend with the engine's interface and its parameter blocks on the host
            params = list(engine.params)
            self.split = int(engine.split) if len(params) == 2 else None
            m = torch.full((self.N,), float(params[0].max_episode))
            if self.split:
                m[self.split:] = float(params[1].max_episode)
            self._max_episode = m.to(self.record.device)

    def zero(self):
        self.record.zero_()

    def update(self, rew, resets, episode_cap: int = 0):
        """One step: rew (N,) float32 and resets (N,) int64 as step() returned them; the goal flag is the engine's goal_reset_buf."""
        e, torch = self.engine, self.torch
        if self._native:
            rew = e._f32(rew, (self.N,))
            assert resets.dtype == torch.int64 and resets.is_contiguous() and resets.device == e.device and tuple(resets.shape) == (self.N,)
            with torch.cuda.device(e.device):
                e._check(e.lib.lm_episode_update(e._h, Engine._p(rew), Engine._p(resets), Engine._p(self.record), int(episode_cap), e._stream()))
            return
        R = self.record
        live = torch.ones(self.N, dtype=torch.bool, device=R.device) if episode_cap <= 0 else R[2] < float(episode_cap)
        d = (resets != 0) & live
        g = e.cnt[2].to(R.device) != 0
        ret = torch.where(live, R[0] + rew.to(R.device, torch.float32), R[0]); length = torch.where(live, R[1] + 1.0, R[1])
        one = d.to(torch.float32)
        R[2] += one; R[3] = torch.where(d, R[3] + ret, R[3]); R[4] = torch.where(d, R[4] + length, R[4])
        timeout = length >= (self._max_episode - 1.0)
        R[5] += (d & g).to(torch.float32); R[6] += (d & ~g & timeout).to(torch.float32); R[7] += (d & ~g & ~timeout).to(torch.float32)
        R[8] = torch.where(d, ret, R[8])
        R[0] = torch.where(d, torch.zeros_like(ret), ret); R[1] = torch.where(d, torch.zeros_like(length), length)

    @staticmethod
    def _reduce(rec):
        n = float(rec[2].sum())
        div = lambda x: float(x) / n if n > 0 else float("nan")
        return {"episodes": int(n), "mean_return": div(rec[3].sum()), "mean_length": div(rec[4].sum()), "success_rate": div(rec[5].sum()),
                "timeout_rate": div(rec[6].sum()), "failure_rate": div(rec[7].sum()), "goals": int(rec[5].sum()), "timeouts": int(rec[6].sum()),
                "failures": int(rec[7].sum())}

    def summary(self, split=None):
        """Host reduction in float64 over the envs: episodes, mean_return, mean_length, success_rate (goal / episodes), timeout_rate,
        failure_rate (and the three counts).  With `split` (the first env of a co-training engine's second block) the same per half under
        "loco" and "mani"."""
        rec = self.record.detach().cpu().double().numpy()
        out = self._reduce(rec)
        split = self.split if split is None else split
        if split:
            out["loco"] = self._reduce(rec[:, :split]); out["mani"] = self._reduce(rec[:, split:])
        return out

    def summary_by(self, groups):
        """The same host reduction per group: `groups` is an int (N,) array / tensor of group ids; returns {id: summary of the envs with that
        id}, ids ascending (what an evaluation sweep reads: one group per grid point)."""
        return EpisodeRecord.reduce_by(self.record.detach().cpu().double().numpy(), groups)

    @staticmethod
    def reduce_by(rec, groups):
        if hasattr(groups, "detach"):
            groups = groups.detach().cpu().numpy()
        g = np.asarray(groups)
        if g.shape != (rec.shape[1],) or not np.issubdtype(g.dtype, np.integer):
            raise ValueError(f"groups: an integer array of shape ({rec.shape[1]},) is needed, got {g.dtype} {g.shape}")
        return {int(k): EpisodeRecord._reduce(rec[:, g == k]) for k in np.unique(g)}


class TrajectoryRecord:
    """The trajectory record of include/lm_policy.h: one row of 64 floats per control step for each of K tracked envs - q, qd, the free body's
    pose (base or plate), the applied actions, the foot tips in the base frame, the goal, reward, done and the counters (COLUMNS) - a copy
    of what stands in the engine after the step.  Owns rows (K, max_rows, 64) float32, header (K, 4) int32 {rows written, episodes completed,
    rows dropped, 0} and the id tensor, on the engine's device.  Hand it to a Rollout (trajectory_record=) or call update() after every
    engine step; zero() starts a measurement (zero it when every env is about to reset and episode_cap = 1 records what the reference's
    RECORD_JOINT does).  On an engine without the C library (CPU tensors: the oracle backend of the tests) update() applies the same rule
    in torch."""

    COLUMNS = dict(q=slice(0, 12), qd=slice(12, 24), free_body=slice(24, 31), last_actions=slice(31, 43), last_tip=slice(43, 55), goal=slice(55, 59),
                   reward=slice(59, 60), done=slice(60, 61), goal_reset=slice(61, 62), progress=slice(62, 63), episode_count=slice(63, 64))

    def __init__(self, engine, env_ids, max_rows: int, episode_cap: int = 1):
        import torch
        self.torch, self.engine, self.N = torch, engine, int(engine.num_envs)
        ids = [int(e) for e in env_ids]
        if not 1 <= len(ids) <= TRAJ_MAX_ENVS:
            raise ValueError(f"a trajectory record tracks 1 .. {TRAJ_MAX_ENVS} envs, not {len(ids)}")
        if len(set(ids)) != len(ids):
            raise ValueError("a trajectory record's env ids must be distinct")
        if min(ids) < 0 or max(ids) >= self.N:
            raise ValueError(f"env ids must lie in [0, {self.N})")
        if int(max_rows) < 1:
            raise ValueError("max_rows must be at least 1")
        self.env_ids, self.K, self.max_rows, self.episode_cap = ids, len(ids), int(max_rows), max(int(episode_cap), 0)
        dev = engine.cnt.device
        self.rows = torch.zeros((self.K, self.max_rows, TRAJ_COLS), dtype=torch.float32, device=dev)
        self.header = torch.zeros((self.K, 4), dtype=torch.int32, device=dev)
        self.ids = torch.tensor(ids, dtype=torch.int32, device=dev)
        self._native = hasattr(engine, "lib") and hasattr(engine, "_h")
        if not self._native:          # a backend with the engine's interface and its parameter blocks on the host: the column -> state row map in torch
            params = list(engine.params)
            split = int(engine.split) if len(params) == 2 else self.N
            src = torch.empty((self.K, 59), dtype=torch.int64)
            for k, e in enumerate(ids):
                fb = ROW["base_pos"] if int(params[1 if e >= split else 0].mode) == 0 else ROW["plate_pos"]
                src[k] = torch.tensor([ROW["q"] + c for c in range(12)] + [ROW["qd"] + c for c in range(12)] + [fb + c for c in range(7)] +
                                      [ROW["last_actions"] + c for c in range(12)] + [ROW["last_tip"] + c for c in range(12)] + [ROW["goal"] + c for c in range(4)])
            self._src = src.to(dev)

    def zero(self):
        self.rows.zero_(); self.header.zero_()

    def update(self, rew, resets):
        """One step: rew (N,) float32 and resets (N,) int64 as step() returned them; everything else is read from the engine."""
        e, torch = self.engine, self.torch
        if self._native:
            rew = e._f32(rew, (self.N,))
            assert resets.dtype == torch.int64 and resets.is_contiguous() and resets.device == e.device and tuple(resets.shape) == (self.N,)
            with torch.cuda.device(e.device):
                e._check(e.lib.lm_trajectory_update(e._h, Engine._p(self.ids), self.K, Engine._p(rew), Engine._p(resets), Engine._p(self.rows), Engine._p(self.header),
                                                    self.max_rows, self.episode_cap, e._stream()))
            return
        ids = self.ids.long()
        state, cnt = e.state.to(self.rows.device), e.cnt.to(self.rows.device)
        row = torch.empty((self.K, TRAJ_COLS), dtype=torch.float32, device=self.rows.device)
        row[:, :59] = state[self._src, ids[:, None]]
        done = resets.to(self.rows.device)[ids] != 0
        row[:, 59] = rew.to(self.rows.device, torch.float32)[ids]; row[:, 60] = done.float(); row[:, 61] = (cnt[2, ids] != 0).float()
        row[:, 62] = cnt[4, ids].float(); row[:, 63] = cnt[5, ids].float()
        H = self.header
        live = torch.ones(self.K, dtype=torch.bool, device=H.device) if self.episode_cap <= 0 else H[:, 1] < self.episode_cap
        room = live & (H[:, 0] < self.max_rows)
        k = torch.nonzero(room).reshape(-1)
        self.rows[k, H[k, 0].long()] = row[k]
        H[:, 0] += room.int(); H[:, 2] += (live & ~room).int(); H[:, 1] += (live & done).int()

    def episodes(self, slot: int):
        """The rows of one slot cut at the done flags: a list of dicts of named numpy arrays (COLUMNS; single columns as (L,) vectors) with
        "complete" (the episode's terminal row was recorded) and "truncated" (rows of this slot were dropped: the last episode is cut short)."""
        hdr = self.header[slot].cpu().numpy()
        rows = self.rows[slot, :int(hdr[0])].cpu().numpy()
        ends = np.nonzero(rows[:, 60] != 0)[0].tolist()
        cuts = [0] + [i + 1 for i in ends]
        if cuts[-1] < len(rows):
            cuts.append(len(rows))
        out = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            ep = {name: (rows[a:b, sl] if sl.stop - sl.start > 1 else rows[a:b, sl.start]) for name, sl in self.COLUMNS.items()}
            ep["complete"] = bool(rows[b - 1, 60] != 0)
            ep["truncated"] = bool(hdr[2] > 0) and b == len(rows)
            out.append(ep)
        return out

    def save_npy(self, directory: str, prefix: str = "trajectory"):
        """Per tracked env e: <prefix>_env<e>.npy - the first recorded episode's q as float32 (L, 12), the format of the reference's recordings -
        and <prefix>_env<e>.npz - every named column of every recorded episode (<name>_<episode index>) plus the slot's header.  Returns the
        .npy paths."""
        os.makedirs(directory, exist_ok=True)
        paths = []
        for slot, e in enumerate(self.env_ids):
            eps = self.episodes(slot)
            base = os.path.join(directory, f"{prefix}_env{e}")
            q = eps[0]["q"] if eps else np.zeros((0, 12), dtype=np.float32)
            np.save(base + ".npy", np.ascontiguousarray(q, dtype=np.float32))
            arrays = {"header": self.header[slot].cpu().numpy(), "env": np.int32(e), "episodes": np.int32(len(eps))}
            for i, ep in enumerate(eps):
                for name in self.COLUMNS:
                    arrays[f"{name}_{i}"] = ep[name]
            np.savez(base + ".npz", **arrays)
            paths.append(base + ".npy")
        return paths


class ReplayRecord:
    """The replay record of include/lm_policy.h: a float (32, N) tensor on the engine's device - per env how far the replay of its recording
    got, how it ended and how close the joints and the orientation error stayed to the recording (rows: REPLAY).  A ReplayPlan fills it
    (plan.run(record), or record.update(plan, s, ...) after every engine step); zero() starts a measurement.  On an engine without the C
    library (CPU tensors: the oracle backend of the tests) update() applies the same rule in torch, in fp32 and in the order of the header."""

    def __init__(self, engine):
        import torch
        self.torch, self.engine, self.N = torch, engine, int(engine.num_envs)
        self.record = torch.empty((REPLAY_ROWS, self.N), dtype=torch.float32, device=engine.cnt.device)
        self._native = hasattr(engine, "lib") and hasattr(engine, "_h")
        self.full = None          # joint displacement of a saturated action: set by the plan that fills the record (summary()'s `early` is in its units)
        self.zero()

    def zero(self):
        self.record.zero_()
        self.record[REPLAY["done_at"]] = -1.0; self.record[REPLAY["first_succ"]] = -1.0; self.record[REPLAY["min_v2"]] = float("inf")

    def update(self, plan, s: int, obs, rew, actions_next):
        """After engine step number s (0: the reset step): obs (N, 64) - on a PD plan (N, engine.num_obs) - and rew (N,) as that step wrote
        them; actions_next (N, 12) receives the actions of step s + 1 (it may be the tensor step s read)."""
        e, torch = self.engine, self.torch
        assert plan.engine is e, "the plan drives another engine"
        self.full = plan.full
        if self._native:
            e._f32(obs, (self.N, e.num_obs if plan.pd else NUM_OBS)); e._f32(rew, (self.N,)); e._f32(actions_next, (self.N, NUM_ACTIONS))
            with torch.cuda.device(e.device):
                e._check(e.lib.lm_replay_update(plan._h, int(s), Engine._p(obs), Engine._p(rew), Engine._p(self.record), Engine._p(actions_next), e._stream()))
            return
        R = self.record; dev = R.device; s = int(s)
        f32 = lambda x: x.to(dev, torch.float32)
        r = plan.env_rec_t.to(dev).long(); part = r >= 0; rr = r.clamp(min=0)
        T = plan.len_t.to(dev).long()[rr]
        live = part & (R[1] == 0) & (s < T + plan.hold)
        q = f32(e.state[ROW["q"]:ROW["q"] + 12]); o = f32(obs); rw = f32(rew)
        v2 = (o[:, 7] * o[:, 7] + o[:, 8] * o[:, 8]) + o[:, 9] * o[:, 9]
        rec = plan.rec_t.to(dev); row = lambda k: rec[rr, min(max(k, 0), plan.T_max - 1)].T           # (12, N); only read where row k exists
        put = lambda i, mask, val: R.__setitem__(i, torch.where(mask, val, R[i]))
        seqsum = lambda x: sum((x[j] for j in range(1, 12)), x[0])          # j = 0 .. 11, in order
        inrec = live & (s < T)
        rs = row(s); d = q - rs; ad = d.abs(); m = ad.max(0).values
        if s == 0:
            put(4, inrec, m); put(14, inrec, v2)
        put(5, inrec, torch.maximum(R[5], m)); put(15, inrec, R[15] + seqsum(ad)); put(6, inrec, R[6] + seqsum(d * d))
        if s >= 1:
            ej = ((q - R[16:28]) - (rs - row(s - 1))).abs()
            put(7, inrec, R[7] + (ej < plan.track_tol).sum(0).to(torch.float32))
            if s <= 4:
                put(8, inrec, R[8] + seqsum(ej))
        win = s >= T - plan.window_rows; ok = inrec & (v2 <= plan.v2_thresh)
        put(9, ok & (R[9] < 0), torch.full_like(v2, float(s))); put(10, ok & win, R[10] + 1.0)
        put(11, inrec, torch.minimum(R[11], v2)); put(13, inrec & win, R[13] + rw); put(0, inrec, R[0] + 1.0)
        R[16:28] = torch.where(inrec[None], q, R[16:28])
        put(12, live, R[12] + rw)
        cnt = e.cnt.to(dev); fin = live & (cnt[3] != 0)
        put(1, fin, torch.ones_like(v2)); put(2, fin, torch.full_like(v2, float(s))); put(3, fin, (cnt[2] != 0).to(torch.float32))
        go = live & ~fin & (s + 1 < T)
        if plan.pd:
            cmd = plan.act_t.to(dev); crow = lambda k: cmd[rr, min(max(k, 0), plan.T_max - 1)].T          # (12, N); only read where row k exists
            if plan.cmd_mode == REPLAY_CMD_TARGETS:
                def se_command(t):          # joint targets -> the swing / extension command of variants 1 / 2 (the inverse of the step's targets)
                    c = t.clone()
                    for l in range(4):
                        c[4 + 2 * l] = 0.5 * (t[4 + 2 * l] + t[5 + 2 * l]); c[5 + 2 * l] = t[4 + 2 * l] - t[5 + 2 * l]
                    return c
                secmd = plan.variant_t.to(dev) >= 1
                se = torch.where(secmd[None], f32(e.state[ROW_SE:ROW_SE + 12]), torch.zeros_like(q))
                if s >= 1:
                    put(REPLAY_CMD_ERR, inrec & secmd, torch.maximum(R[REPLAY_CMD_ERR], (se_command(crow(s)) - se).abs().max(0).values))
                t = crow(s + 1)
                raw = (torch.where(secmd[None], se_command(t), t) - se) * plan.inv_scale_t.to(dev)[None]
                put(REPLAY_SATURATED, go, R[REPLAY_SATURATED] + (raw.abs() > 1.0).sum(0).to(torch.float32))
                nxt = raw.clamp(-1.0, 1.0)
            else:
                nxt = crow(s + 1)
        else:
            nxt = ((row(s + 1) - q) * plan.inv_full).clamp(-1.0, 1.0) if plan.servo else plan.act_t.to(dev)[rr, min(s + 1, plan.T_max - 1)].T
        actions_next.copy_(torch.where(go[None], nxt, torch.zeros_like(nxt)).T.to(actions_next.device))

    def summary(self):
        """Host reduction per env, the quantities of the project's host replay (numpy arrays of shape (N,); envs that took no part have rows 0):
        rows, done_at and first_succ (-1: never), goal, row0_err, qerr, rms and mean_abs (joint error over the recorded rows), tracked (share
        of joint-steps within track_tol), early (mean joint-step error of the first four steps in units of a saturated action; needs the
        plan's `full`; nan on a PD plan), in_window, min_rd and rd_first = 2 asin(sqrt(v2)), return and window_return; saturated (joint-steps
        whose action left [-1, 1] before the clamp) and cmd_err (largest distance of the engine's held command from the logged one, rad):
        both zero unless a PD plan ran in targets mode."""
        rec = self.record.detach().cpu().double().numpy()
        rows = rec[0]; steps = np.maximum(rows - 1.0, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            rd = lambda v2: 2.0 * np.arcsin(np.sqrt(np.clip(v2, 0.0, 1.0)))
            return dict(rows=rows.astype(np.int64), finished=rec[1] != 0, done_at=rec[2].astype(np.int64), goal=rec[3].astype(np.int64), row0_err=rec[4], qerr=rec[5],
                        rms=np.sqrt(rec[6] / (12.0 * rows)), mean_abs=rec[15] / (12.0 * rows), tracked=rec[7] / (12.0 * steps),
                        early=rec[8] / (12.0 * np.minimum(4.0, steps) * (self.full if self.full else np.nan)), first_succ=rec[9].astype(np.int64),
                        in_window=rec[10].astype(np.int64), min_rd=rd(rec[11]), rd_first=rd(rec[14]), window_return=rec[13],
                        saturated=rec[REPLAY_SATURATED].astype(np.int64), cmd_err=rec[REPLAY_CMD_ERR], **{"return": rec[12]})


class ReplayPlan:
    """A replay plan of include/lm_policy.h: N envs of `engine` driven along recorded joint trajectories and scored against them on the device.
    `recordings` is a list of (L, 12) arrays (joint order of robot.joint_positions: the reference's RECORD_JOINT files, TrajectoryRecord.save_npy);
    `env_rec` (N,) names the recording each env replays, -1 for an env that takes no part.  `actions` (a list of (L, 12) arrays: the action
    applied at every row, row 0 the reset step's) defaults to the actions recovered from the recording, [0, clip(diff(rec) / full, +-1)] with
    full = act_scale x control period of the engine's blocks, computed in float64 and cast to float32.  servo=True steers every joint back onto
    the recording each step instead; `hold` zero-action rows follow a recording so that a late success streak can complete; `window_rows` and
    `succ_thresh` are the task's success window (rows and rot_dist in radians), `track_tol` the joint-step error that counts as tracked.
    PD-actuator engines (every block variant 1, variant 2, or variant 0 in position drive; lm_replay_create_pd) replay a command log and need
    one of: `actions` (the logged action of every row; TrajectoryRecord's last_actions), `targets` (a list of (L, 12) arrays: the joint position
    targets commanded for every row, in the recordings' joint order) or servo=True, which here means targets = the recordings themselves, so
    that each step commands the recorded joints.  With none of the three a PD engine is refused as before; `targets` on a velocity-drive
    engine is a ValueError.  A PD plan has no `full` (summary()'s `early` is nan).  On an engine without the C library (the oracle backend of
    the tests) the plan keeps its tables as torch tensors and ReplayRecord.update applies the rule in torch."""

    def __init__(self, engine, recordings, env_rec, actions=None, servo: bool = False, hold: int = 2, window_rows: int = 17, succ_thresh: float = 0.15,
                 track_tol: float = 1e-3, targets=None):
        import torch
        self.torch, self.engine, self.N = torch, engine, int(engine.num_envs)
        recs = [np.asarray(a, dtype=np.float64) for a in recordings]
        if not recs or any(a.ndim != 2 or a.shape[1] != NUM_ACTIONS or a.shape[0] < 1 for a in recs):
            raise ValueError("recordings: a non-empty list of (L, 12) arrays is needed")
        is_pd = lambda p: int(p.variant) in (1, 2) or (int(p.variant) == 0 and int(p.drive_mode) == 1)
        pd_engine = all(is_pd(p) for p in engine.params)
        if targets is not None and not pd_engine:
            raise ValueError("targets: joint position targets drive PD-actuator blocks only (variant 1, variant 2, or variant 0 in position drive); "
                             "this engine has a block in velocity or effort drive")
        self.pd = pd_engine and (actions is not None or targets is not None or bool(servo))
        if self.pd:
            self._init_pd(recs, env_rec, actions, targets, servo, hold, window_rows, succ_thresh, track_tol)
            return
        fulls = {float(p.act_scale) * float(p.ctrl_dt) for p in engine.params}
        if len(fulls) != 1:
            raise ValueError(f"the engine's blocks differ in act_scale x control period ({sorted(fulls)}): one plan scales every action alike")
        self.full = fulls.pop()
        if actions is None:
            acts = [np.concatenate([np.zeros((1, NUM_ACTIONS)), np.clip(np.diff(a, axis=0) / self.full, -1.0, 1.0)]) for a in recs]
        else:
            acts = [np.asarray(a, dtype=np.float64) for a in actions]
            if len(acts) != len(recs) or any(a.shape != b.shape for a, b in zip(acts, recs)):
                raise ValueError("actions: one (L, 12) array per recording is needed, of the recording's shape")
        ids = np.asarray(env_rec.detach().cpu().numpy() if hasattr(env_rec, "detach") else env_rec)
        if ids.shape != (self.N,) or not np.issubdtype(ids.dtype, np.integer):
            raise ValueError(f"env_rec: an integer array of shape ({self.N},) is needed, got {ids.dtype} {ids.shape}")
        self.R, self.T_max = len(recs), max(a.shape[0] for a in recs)
        rec = np.zeros((self.R, self.T_max, NUM_ACTIONS), dtype=np.float32); act = np.zeros_like(rec)
        for k, (a, b) in enumerate(zip(recs, acts)):
            rec[k, :a.shape[0]] = a; act[k, :a.shape[0]] = b
        lens = np.asarray([a.shape[0] for a in recs], dtype=np.int32); ids = np.ascontiguousarray(ids, dtype=np.int32)
        self.servo, self.hold, self.window_rows = bool(servo), int(hold), int(window_rows)
        self.inv_full = float(np.float32(1.0 / self.full)); self.v2_thresh = float(np.float32(np.sin(0.5 * float(succ_thresh)) ** 2)); self.track_tol = float(np.float32(track_tol))
        dev = engine.cnt.device
        self.rec_t, self.act_t = torch.from_numpy(rec).to(dev), torch.from_numpy(act).to(dev)
        self.len_t, self.env_rec_t = torch.from_numpy(lens).to(dev), torch.from_numpy(ids).to(dev)
        self._native = hasattr(engine, "lib") and hasattr(engine, "_h")
        self._h = C.c_void_p()
        if self._native:
            p = lambda a: a.ctypes.data_as(C.c_void_p)
            with torch.cuda.device(engine.device):
                engine._check(engine.lib.lm_replay_create(C.byref(self._h), engine._h, p(rec), p(act), p(lens), self.R, self.T_max, p(ids), int(self.servo), self.hold,
                                                          self.window_rows, self.inv_full, self.v2_thresh, self.track_tol))
            self.steps = int(engine.lib.lm_replay_steps(self._h))
        else:          # the library's refusals, for a backend without it
            if any(int(p.variant) != 0 or int(p.drive_mode) != 0 or int(p.num_obs) != NUM_OBS for p in engine.params):
                raise ValueError("every block must be variant 0 in velocity drive with 64-wide observations (PD targets are not joint-rate actions)")
            if not np.isfinite(rec).all() or not np.isfinite(act).all():
                raise ValueError("a table entry is not finite")
            if not 0 <= self.hold <= 8 or self.window_rows < 1 or (lens < self.window_rows).any() or ids.min() < -1 or ids.max() >= self.R:
                raise ValueError("hold must be in [0, 8], every recording at least window_rows long and every id in [-1, R)")
            self.steps = int(max((int(lens[r]) + self.hold for r in set(ids[ids >= 0].tolist())), default=0))

    def _init_pd(self, recs, env_rec, actions, targets, servo, hold, window_rows, succ_thresh, track_tol):
        """A PD plan: the command table (actions or targets) instead of the action table, the scales read from the engine's blocks."""
        torch, engine = self.torch, self.engine
        if (actions is not None) + (targets is not None) + bool(servo) != 1:
            raise ValueError("a PD engine replays ONE command log: give actions=, targets= or servo=True (targets = the recordings), not several")
        self.cmd_mode = REPLAY_CMD_ACTIONS if actions is not None else REPLAY_CMD_TARGETS
        name = "actions" if actions is not None else "targets"
        cmds = recs if servo else [np.asarray(a, dtype=np.float64) for a in (actions if actions is not None else targets)]
        if len(cmds) != len(recs) or any(a.shape != b.shape for a, b in zip(cmds, recs)):
            raise ValueError(f"{name}: one (L, 12) array per recording is needed, of the recording's shape")
        ids = np.asarray(env_rec.detach().cpu().numpy() if hasattr(env_rec, "detach") else env_rec)
        if ids.shape != (self.N,) or not np.issubdtype(ids.dtype, np.integer):
            raise ValueError(f"env_rec: an integer array of shape ({self.N},) is needed, got {ids.dtype} {ids.shape}")
        self.R, self.T_max = len(recs), max(a.shape[0] for a in recs)
        rec = np.zeros((self.R, self.T_max, NUM_ACTIONS), dtype=np.float32); cmd = np.zeros_like(rec)
        for k, (a, b) in enumerate(zip(recs, cmds)):
            rec[k, :a.shape[0]] = a; cmd[k, :a.shape[0]] = b
        lens = np.asarray([a.shape[0] for a in recs], dtype=np.int32); ids = np.ascontiguousarray(ids, dtype=np.int32)
        self.servo, self.hold, self.window_rows = bool(servo), int(hold), int(window_rows)
        self.full, self.inv_full = None, float("nan")
        self.v2_thresh = float(np.float32(np.sin(0.5 * float(succ_thresh)) ** 2)); self.track_tol = float(np.float32(track_tol))
        dev = engine.cnt.device
        self.rec_t, self.act_t = torch.from_numpy(rec).to(dev), torch.from_numpy(cmd).to(dev)
        self.len_t, self.env_rec_t = torch.from_numpy(lens).to(dev), torch.from_numpy(ids).to(dev)
        self._native = hasattr(engine, "lib") and hasattr(engine, "_h")
        self._h = C.c_void_p()
        # the plan's per-env view of the blocks, as the library forms it: the variant and the reciprocal of the action scale, in float, once
        params = list(engine.params)
        split = (engine.split_env if self._native else int(engine.split)) if len(params) == 2 else None
        block = [params[1 if (split and e >= split) else 0] for e in range(self.N)]
        inv = np.asarray([np.float32(1.0) / np.float32(b.act_scale_se if int(b.variant) >= 1 else b.act_scale) for b in block], dtype=np.float32)
        self.variant_t = torch.tensor([int(b.variant) for b in block], dtype=torch.int64, device=dev)
        self.inv_scale_t = torch.from_numpy(inv).to(dev)
        if self._native:
            p = lambda a: a.ctypes.data_as(C.c_void_p)
            with torch.cuda.device(engine.device):
                engine._check(engine.lib.lm_replay_create_pd(C.byref(self._h), engine._h, p(rec), p(cmd), p(lens), self.R, self.T_max, p(ids), self.cmd_mode, self.hold,
                                                             self.window_rows, self.v2_thresh, self.track_tol))
            self.steps = int(engine.lib.lm_replay_steps(self._h))
            return
        # the library's refusals, for a backend without it
        if not np.isfinite(rec).all() or not np.isfinite(cmd).all():
            raise ValueError("a table entry is not finite")
        if not 0 <= self.hold <= 8 or self.window_rows < 1 or (lens < self.window_rows).any() or ids.min() < -1 or ids.max() >= self.R:
            raise ValueError("hold must be in [0, 8], every recording at least window_rows long and every id in [-1, R)")
        self.steps = int(max((int(lens[r]) + self.hold for r in set(ids[ids >= 0].tolist())), default=0))
        if not np.isfinite(inv).all():
            raise ValueError("a block whose action scale has no finite reciprocal")

    def run(self, record: ReplayRecord, zero: bool = True):
        """Replay on an engine whose envs are all about to reset (a fresh engine, or after reset_all()): for s = 0 .. steps - 1, Engine.step(actions)
        and then the record update, which also writes the next actions; nothing waits for the host inside the loop.  Returns the record."""
        e, torch = self.engine, self.torch
        dev = e.cnt.device
        if zero:
            record.zero()
        actions = torch.zeros((self.N, NUM_ACTIONS), dtype=torch.float32, device=dev)
        obs = torch.empty((self.N, int(e.num_obs) if self.pd else NUM_OBS), dtype=torch.float32, device=dev); rew = torch.empty((self.N,), dtype=torch.float32, device=dev)
        for s in range(self.steps):
            e.step(actions, out_obs=obs, out_rew=rew)
            record.update(self, s, obs, rew, actions)
        return record

    def close(self):
        if self._h:
            self.engine.lib.lm_replay_destroy(self._h); self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
