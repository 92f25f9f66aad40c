"""Domain randomisation front end (reference: utils/domain_randomization/randomize.py:39-578).

The reference's `Randomizer` reads the `domain_randomization` block of the task YAML
(cfg/task/QuadrupedPoseControl.yaml:102-173), adds observation / action noise in Python (:212-306) and registers the physics
attributes with omni.replicator.isaac.  Here the same YAML block is compiled into the engine's parameter block
(`lm_params.dr[]`, include/lm_engine.h) and *everything is sampled inside the one `lm_step` launch* (kernel `k_step_dr`): action
noise before the clipActions clamp, per-env gravity / base-link force / max efforts / max joint velocities for the control step,
observation noise on `obs_buf` before the clipObservations clamp.  The class keeps the reference's attribute and method names so
that the task / wrapper code reads the same (`randomize`, `min_frequency`, `set_up_domain_randomization`,
`apply_on_startup_domain_randomization`, `apply_actions_randomization`, `apply_observations_randomization`).

Supported entries (everything the reference's YAMLs enable):
    observations / actions        on_reset + on_interval, additive | scaling, gaussian | uniform | loguniform
    simulation.gravity            on_interval or on_reset, additive | scaling | direct, per-component parameters
    rigid_prim_views.<base link>.force                 "
    articulation_views.<robot>.max_efforts             "   (scalar parameters, one draw per joint)
    articulation_views.<robot>.joint_max_velocities    "
    articulation_views.<robot>.damping                 "   (the viscous joint damping of the PD-actuator tasks; no effect on velocity-drive tasks,
                                                           whose joint_damping is 0)
    articulation_views.<robot>.joint_friction          accepted and ignored with a warning (joint friction itself is not modelled)
    articulation_views.<robot>.scale on_startup        accepted with a warning: factors drawn and recorded, not applied (see
                                                       apply_on_startup_domain_randomization: the reference's call does not rescale the links either)
    articulation_views.<robot>.material_properties     on_startup | on_reset | on_interval, [static, dynamic, restitution] parameters,
    rigid_prim_views.plate.material_properties         optional num_buckets: the contact friction of the feet / of the plate per env
                                                       (EngineParams.dr_mat).  Only the dynamic component enters; a
                                                       static or restitution component that would change warns (not modelled)
    articulation_views.<robot>.joint_positions         on_reset, additive | scaling | direct, scalar parameters: the 12 driven joints' reset pose
    articulation_views.<robot>.joint_velocities        on_reset, additive | direct, scalar parameters: their reset velocity (nominal 0)
    articulation_views.<robot>.position                on_reset, additive | scaling | direct, per-component parameters: the base's reset position
    articulation_views.<robot>.orientation             on_reset, additive | direct, per-component Euler angles (roll, pitch, yaw): its reset orientation
    rigid_prim_views.plate.position / .orientation     the same for the plate of the manipulation blocks (the robot is fixed there)
                                                       (EngineParams.dr_reset; DESIGN.md 3.6: drawn inside the step launch at every reset that
                                                       passes min_frequency; no clamping to the joint ranges)
    rigid_prim_views.plate.mass                        on_startup | on_reset | on_interval, additive | scaling | direct, [a, b]: the plate's mass per
                                                       env (manipulation blocks).  Mass only: COM and inertia about the COM stay
    rigid_prim_views.plate.density                     on_startup, scaling only: a factor on the plate's mass AND inertia, applied before `mass`
                                                       (the URDF gives no volume, so there is no nominal density to add to or to replace)
    articulation_views.<robot>.body_masses             on_startup | on_reset | on_interval, additive | scaling | direct: the masses of the 21 bodies,
                                                       one draw per body; [a, b] for all bodies or [[21 values], [21 values]] in
                                                       RobotModel.body_names order.  Mass only.  Component 0 is the base link: a payload
                                                       (EngineParams.dr_mass; DESIGN.md 3.6: drawn inside the step launch, floored at 0.05 x nominal;
                                                       a uniform / loguniform range that reaches a non-positive mass is refused; parity with the
                                                       replicator is unpinned, as for every physics attribute)
    articulation_views.<robot>.joint_kps               on_startup | on_reset | on_interval, additive | scaling | direct, [a, b]: the position gain of the
                                                       12 driven joints, ONE draw per env (nominal: the task's kp).  PD-actuator tasks and
                                                       position control; refused in velocity / effort control (there is no position gain)
    articulation_views.<robot>.joint_kds               the same for the velocity gain kd; every task except effort control (gains off)
    articulation_views.<robot>.command_latency         on_startup | on_reset | on_interval, additive | direct, [a, b] in sub-steps: the first
                                                       d = clamp(floor(draw), 0, sub-steps per step) sub-steps of a control step still follow the
                                                       previous command.  PD-actuator tasks only
                                                       (EngineParams.dr_actuator; DESIGN.md 3.6: drawn inside the step launch, gains floored at 0.05 x
                                                       nominal; a uniform / loguniform range that reaches a non-positive gain is refused)
Anything else (mass / density of other rigid-prim views - the base link's included: use body_masses -, body_inertias, material_properties of
other views, stiffness ...) raises NotImplementedError when `randomize: True` - a silently ignored randomisation would be worse than a loud one."""
from __future__ import annotations

from typing import List

import numpy as np

from ...engine_config import (DR_ACT_INTERVAL, DR_ACT_RESET, DR_ACTUATOR_CHANNELS, DR_ACTUATOR_KD, DR_ACTUATOR_KP, DR_ACTUATOR_LATENCY, DR_BASE_FORCE, DR_CHANNELS, DR_DISTRIBUTIONS, DR_GRAVITY, DR_JOINT_DAMPING, DR_MAT_OTHER,
                              DR_MAT_ROBOT, DR_MASS_BODIES, DR_MASS_CHANNELS, DR_MASS_FLOOR, DR_MASS_PLATE, DR_MASS_PLATE_DENSITY, DR_MAX_EFFORT, DR_MAX_VELOCITY, DR_OBS_INTERVAL, DR_OBS_RESET, DR_ON_STARTUP, DR_OPERATIONS, DR_RESET_CHANNELS,
                              DR_RESET_JOINT_POS, DR_RESET_JOINT_VEL, DR_RESET_ORIENTATION, DR_RESET_POSITION, MODE_LOCO, MODE_MANI, NUM_BODIES, DRChannel)

_ON_RESET_KEYS = ("operation", "distribution", "distribution_parameters")
_ON_INTERVAL_KEYS = ("frequency_interval", "operation", "distribution", "distribution_parameters")


def _channel(where: str, entry: dict, trigger: str, vector: bool) -> DRChannel:
    need = _ON_INTERVAL_KEYS if trigger == "on_interval" else _ON_RESET_KEYS
    if not set(need).issubset(entry.keys()):          # randomize.py:182-190
        raise ValueError(f"Please ensure the following randomization parameters for {where} {trigger} are provided: " + ", ".join(need) + ".")
    op, dist = str(entry["operation"]), str(entry["distribution"])
    if op not in DR_OPERATIONS or dist not in DR_DISTRIBUTIONS:
        raise ValueError(f"{where} {trigger}: unsupported operation {op!r} or distribution {dist!r}")
    prm = np.asarray(entry["distribution_parameters"], dtype=np.float64)
    if vector:
        if prm.shape != (2, 3):
            raise ValueError(f"{where} {trigger}: distribution_parameters must be [[3 values], [3 values]]")
        p0, p1 = prm[0].tolist(), prm[1].tolist()
    else:
        if prm.shape != (2,):
            raise ValueError(f"{where} {trigger}: distribution_parameters must be [a, b]")
        p0, p1 = [float(prm[0])] * 3, [float(prm[1])] * 3
    interval = int(entry["frequency_interval"]) if trigger == "on_interval" else 0
    if trigger == "on_interval" and interval < 1:
        raise ValueError(f"{where}: frequency_interval must be >= 1")
    return DRChannel(enabled=1, operation=DR_OPERATIONS[op], distribution=DR_DISTRIBUTIONS[dist], interval=interval, p0=p0, p1=p1)


_MAT_COMPONENTS = ("static", "dynamic", "restitution")
PLATE_VIEW = "plate"          # the plate's RigidPrimView name (reference objects/plate.py:8, objects/base/rigid_object.py:30)


def _degenerate(dist: int, p0: float, p1: float):
    """The one value a distribution can take, or None (gaussian: std 0; uniform / loguniform: low == high)."""
    if dist == DR_DISTRIBUTIONS["gaussian"]:
        return p0 if p1 == 0 else None
    return p0 if p0 == p1 else None


def _changes(op: int, dist: int, p0: float, p1: float, nominal: float) -> bool:
    """Whether a channel component would move a quantity from its nominal value."""
    v = _degenerate(dist, p0, p1)
    if op == DR_OPERATIONS["additive"]:
        return v != 0.0
    if op == DR_OPERATIONS["scaling"]:
        return nominal != 0.0 and v != 1.0
    return v != nominal


def _material_channel(where: str, entry: dict, trigger: str):
    """One material_properties trigger -> (DRChannel over [static, dynamic, restitution], num_buckets)."""
    need = _ON_INTERVAL_KEYS if trigger == "on_interval" else _ON_RESET_KEYS
    if entry is None or not set(need).issubset(entry.keys()):          # randomize.py:357-359,376-378
        raise ValueError(f"Please ensure the following randomization parameters for {where} {trigger} are provided: " + ", ".join(need) + ".")
    op, dist = str(entry["operation"]), str(entry["distribution"])
    if op not in DR_OPERATIONS or dist not in DR_DISTRIBUTIONS:
        raise ValueError(f"{where} {trigger}: unsupported operation {op!r} or distribution {dist!r}")
    raw = entry["distribution_parameters"]
    try:
        prm = np.asarray(raw, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{where} {trigger}: distribution_parameters must be numbers, got {raw!r}") from None
    if prm.shape == (2,):          # one pair for all three components (randomize.py:445-447)
        prm = np.repeat(prm[:, None], 3, axis=1)
    if prm.shape != (2, 3) or not np.isfinite(prm).all():
        raise ValueError(f"{where} {trigger}: distribution_parameters must be [[static, dynamic, restitution], [static, dynamic, restitution]] "
                         f"(or [a, b] for all three), got {raw!r}" + (" - operation 'direct' needs the values it sets" if op == "direct" else ""))
    if dist in ("loguniform", "log_uniform") and not (prm > 0).all():
        raise ValueError(f"{where} {trigger}: loguniform parameters must be positive")
    buckets = 0
    if "num_buckets" in entry:          # randomize.py:361-362: optional
        b = entry["num_buckets"]
        if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or b < 1:
            raise ValueError(f"{where} {trigger}: num_buckets must be a positive integer, got {b!r}")
        buckets = int(b)
    interval = {"on_startup": DR_ON_STARTUP, "on_reset": 0}.get(trigger)
    if interval is None:
        interval = int(entry["frequency_interval"])
        if interval < 1:
            raise ValueError(f"{where}: frequency_interval must be >= 1")
    ch = DRChannel(enabled=1, operation=DR_OPERATIONS[op], distribution=DR_DISTRIBUTIONS[dist], interval=interval, p0=prm[0].tolist(), p1=prm[1].tolist())
    return ch, buckets


# reset-state attributes -> (channel, vector parameters, operations that make sense)
_RESET_STATE = {"joint_positions": (DR_RESET_JOINT_POS, False, ("additive", "scaling", "direct")),
                "joint_velocities": (DR_RESET_JOINT_VEL, False, ("additive", "direct")),
                "position": (DR_RESET_POSITION, True, ("additive", "scaling", "direct")),
                "orientation": (DR_RESET_ORIENTATION, True, ("additive", "direct"))}
_RESET_STATE_WHY = {"joint_velocities": "the nominal joint velocity is 0, so scaling it changes nothing",
                    "orientation": "the draw is three Euler angles turned into a quaternion, which is applied after the nominal one (additive) or "
                                   "replaces it (direct); a quaternion is not scaled"}


def _reset_state_channel(where: str, attribute: str, entry: dict) -> DRChannel:
    """One reset-state entry (joint_positions / joint_velocities / position / orientation) -> DRChannel; on_reset is the only trigger."""
    _, vector, ops = _RESET_STATE[attribute]
    if entry is None:
        raise ValueError(f"Randomization parameters for {where} is not provided.")
    other = [t for t in ("on_interval", "on_startup") if t in entry]
    if other or "on_reset" not in entry:
        raise NotImplementedError(f"{where}: the reset state is drawn when an env is reset, so on_reset is its only trigger"
                                  + (f" (got {', '.join(other)})" if other else ""))
    e = entry["on_reset"]
    if e is not None and "operation" in e and str(e["operation"]) in DR_OPERATIONS and str(e["operation"]) not in ops:
        raise ValueError(f"{where} on_reset: operation {e['operation']!r} is refused: {_RESET_STATE_WHY[attribute]}")
    ch = _channel(where, e or {}, "on_reset", vector)
    n = 3 if vector else 1
    if not (np.isfinite(ch.p0[:n]).all() and np.isfinite(ch.p1[:n]).all()):
        raise ValueError(f"{where} on_reset: distribution_parameters must be finite")
    if ch.distribution == DR_DISTRIBUTIONS["loguniform"] and not (min(ch.p0[:n]) > 0 and min(ch.p1[:n]) > 0):
        raise ValueError(f"{where} on_reset: loguniform parameters must be positive")
    return ch


_MASS_REFUSED = ("rigid_prim_views.{view}.{attribute}: only the plate's mass / density are channels of this engine (rigid_prim_views." + PLATE_VIEW +
                 ".mass / .density); the masses of the robot's links - the base link's included, e.g. a payload - are "
                 "articulation_views.<robot>.body_masses, whose component 0 is the base link")
_NO_PLATE = ("rigid_prim_views.{view}.{attribute}: this task has no manipulation block, so there is no plate whose {attribute} could be randomised; "
             "the robot's masses are articulation_views.<robot>.body_masses")


def _mass_channel(where: str, attribute: str, entry: dict):
    """One mass entry (plate `mass` / `density`, `body_masses`) -> (trigger, DRChannel, per-body low / mean, per-body high / std or None)."""
    if entry is None:
        raise ValueError(f"Randomization parameters for {where} is not provided.")
    triggers = [t for t in ("on_startup", "on_reset", "on_interval") if t in entry]
    if len(triggers) != 1:
        raise NotImplementedError(f"{where}: give exactly one of on_startup, on_reset, on_interval")
    trigger = triggers[0]
    e = entry[trigger]
    need = _ON_INTERVAL_KEYS if trigger == "on_interval" else _ON_RESET_KEYS
    if e is None or not set(need).issubset(e.keys()):
        raise ValueError(f"Please ensure the following randomization parameters for {where} {trigger} are provided: " + ", ".join(need) + ".")
    op, dist = str(e["operation"]), str(e["distribution"])
    if op not in DR_OPERATIONS or dist not in DR_DISTRIBUTIONS:
        raise ValueError(f"{where} {trigger}: unsupported operation {op!r} or distribution {dist!r}")
    if attribute == "density":
        why = "the URDF gives the plate's mass and inertia but no volume, so no nominal density exists"
        if trigger != "on_startup":
            raise NotImplementedError(f"{where} {trigger}: density is an on_startup entry (a factor on the plate's mass and inertia, drawn once per env); {why}")
        if op != "scaling":
            raise ValueError(f"{where} {trigger}: operation {op!r} is refused: {why} - only a scaling factor is defined")
    raw = e["distribution_parameters"]
    try:
        prm = np.asarray(raw, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{where} {trigger}: distribution_parameters must be numbers, got {raw!r}") from None
    per_body = attribute == "body_masses" and prm.ndim == 2
    if not (prm.shape == (2,) or (per_body and prm.shape == (2, NUM_BODIES))):
        raise ValueError(f"{where} {trigger}: distribution_parameters must be [a, b]" +
                         (f" or [[{NUM_BODIES} values], [{NUM_BODIES} values]] in RobotModel.body_names order" if attribute == "body_masses" else "") + f", got shape {prm.shape}")
    if not np.isfinite(prm).all():
        raise ValueError(f"{where} {trigger}: distribution_parameters must be finite")
    if DR_DISTRIBUTIONS[dist] == DR_DISTRIBUTIONS["loguniform"] and not (prm > 0).all():
        raise ValueError(f"{where} {trigger}: loguniform parameters must be positive")
    interval = {"on_startup": DR_ON_STARTUP, "on_reset": 0}.get(trigger)
    if interval is None:
        interval = int(e["frequency_interval"])
        if interval < 1:
            raise ValueError(f"{where}: frequency_interval must be >= 1")
    lo, hi = (prm[0], prm[1]) if per_body else (np.full(NUM_BODIES, prm[0]), np.full(NUM_BODIES, prm[1]))
    ch = DRChannel(enabled=1, operation=DR_OPERATIONS[op], distribution=DR_DISTRIBUTIONS[dist], interval=interval,
                   p0=[float(lo[0])] * 3, p1=[float(hi[0])] * 3)
    return trigger, ch, lo.astype(np.float64), hi.astype(np.float64)


def _least_mass(ch: DRChannel, lo: float, hi: float, nominal: float):
    """The least value a bounded distribution (uniform, loguniform) can give a mass of `nominal`; None for the unbounded gaussian (floored)."""
    if ch.distribution == DR_DISTRIBUTIONS["gaussian"]:
        return None
    low = min(lo, hi)
    return nominal + low if ch.operation == DR_OPERATIONS["additive"] else nominal * low if ch.operation == DR_OPERATIONS["scaling"] else low


_ACTUATOR = {"joint_kps": DR_ACTUATOR_KP, "joint_kds": DR_ACTUATOR_KD, "command_latency": DR_ACTUATOR_LATENCY}


def _actuator_channel(where: str, attribute: str, entry: dict):
    """One actuator entry (`joint_kps`, `joint_kds`, `command_latency`) -> (trigger, DRChannel): exactly one trigger, a scalar pair."""
    if entry is None:
        raise ValueError(f"Randomization parameters for {where} is not provided.")
    triggers = [t for t in ("on_startup", "on_reset", "on_interval") if t in entry]
    if len(triggers) != 1:
        raise NotImplementedError(f"{where}: give exactly one of on_startup, on_reset, on_interval")
    trigger = triggers[0]
    e = entry[trigger]
    need = _ON_INTERVAL_KEYS if trigger == "on_interval" else _ON_RESET_KEYS
    if e is None or not set(need).issubset(e.keys()):
        raise ValueError(f"Please ensure the following randomization parameters for {where} {trigger} are provided: " + ", ".join(need) + ".")
    op, dist = str(e["operation"]), str(e["distribution"])
    if op not in DR_OPERATIONS or dist not in DR_DISTRIBUTIONS:
        raise ValueError(f"{where} {trigger}: unsupported operation {op!r} or distribution {dist!r}")
    if attribute == "command_latency" and op == "scaling":
        raise ValueError(f"{where} {trigger}: operation 'scaling' is refused: the nominal latency is 0 sub-steps, so a factor changes nothing - use additive or direct")
    raw = e["distribution_parameters"]
    try:
        prm = np.asarray(raw, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{where} {trigger}: distribution_parameters must be numbers, got {raw!r}") from None
    if prm.shape != (2,):
        raise ValueError(f"{where} {trigger}: distribution_parameters must be [a, b] (one draw per env, applied to the 12 driven joints), got shape {prm.shape}")
    if not np.isfinite(prm).all():
        raise ValueError(f"{where} {trigger}: distribution_parameters must be finite")
    if DR_DISTRIBUTIONS[dist] == DR_DISTRIBUTIONS["loguniform"] and not (prm > 0).all():
        raise ValueError(f"{where} {trigger}: loguniform parameters must be positive")
    interval = {"on_startup": DR_ON_STARTUP, "on_reset": 0}.get(trigger)
    if interval is None:
        interval = int(e["frequency_interval"])
        if interval < 1:
            raise ValueError(f"{where}: frequency_interval must be >= 1")
    return trigger, DRChannel(enabled=1, operation=DR_OPERATIONS[op], distribution=DR_DISTRIBUTIONS[dist], interval=interval,
                              p0=[float(prm[0])] * 3, p1=[float(prm[1])] * 3)


class Randomizer:
    def __init__(self, sim_config):
        self._cfg = sim_config.task_config
        self._config = sim_config.config
        self.randomize = False
        self.min_frequency = 1
        self.active_domain_randomizations = dict()
        self._channels: List[DRChannel] = [DRChannel() for _ in range(DR_CHANNELS)]
        self._mat_channels: List[DRChannel] = [DRChannel(), DRChannel()]          # [robot feet, plate] (EngineParams.dr_mat)
        self._mat_buckets: List[int] = [0, 0]
        # reset-state channels per block mode (EngineParams.dr_reset): the joint entries go to both, position / orientation to the block
        # whose free body they name (articulation_views.<robot>: the base of locomotion blocks; rigid_prim_views.plate: manipulation blocks)
        self._reset_channels = {MODE_LOCO: [DRChannel() for _ in range(DR_RESET_CHANNELS)], MODE_MANI: [DRChannel() for _ in range(DR_RESET_CHANNELS)]}
        # mass channels (EngineParams.dr_mass): [plate mass, plate density, body masses]; the plate's go to manipulation blocks only.  The body
        # channel's parameters per body, in table order
        self._mass_channels: List[DRChannel] = [DRChannel() for _ in range(DR_MASS_CHANNELS)]
        self._mass_body_p0: List[float] = [0.0] * NUM_BODIES
        self._mass_body_p1: List[float] = [0.0] * NUM_BODIES
        # actuator channels (EngineParams.dr_actuator): [kp, kd, command latency], one draw per env; checked against each block's actuator
        # family and gains when the task builds the block (check_actuator)
        self._actuator_channels: List[DRChannel] = [DRChannel() for _ in range(DR_ACTUATOR_CHANNELS)]
        self._actuator_where = {}
        self._observations_dr_params = None
        self._actions_dr_params = None
        self.startup_scales = dict()          # (group, view) -> per-env factors drawn by apply_on_startup_domain_randomization
        dr_config = self._cfg.get("domain_randomization", None)
        if dr_config is not None:
            randomize = dr_config.get("randomize", False)
            randomization_params = dr_config.get("randomization_params", None)
            if randomize and randomization_params is not None:          # randomize.py:52-56
                self.randomize = True
                self.min_frequency = int(dr_config.get("min_frequency", 1))

    # ------------------------------------------------------------------ reference entry points
    def apply_on_startup_domain_randomization(self, task):
        """randomize.py:58-117: scale / mass / density on_startup.

        `articulation_views.<robot>.scale` is the one on_startup entry the reference's YAMLs carry (cfg/task/QuadrupedPoseControl.yaml:167-172,
        uniform [0.98, 1.02]).  In the reference it calls `view.set_local_scales` on the articulation root, which its authors note does not
        scale the robot ("checked; but not scaling the entire robot?", :110 of that YAML): the link geometry, inertias and joint frames PhysX
        simulates are unchanged.  Here the entry is therefore ACCEPTED: the per-env factors are drawn as the reference draws them (one
        synchronised factor per env, torch generator seeded with the config seed, randomize.py:60,308-350) and kept in `startup_scales`
        for inspection, a warning says that they do not enter the dynamics, and the compiled model table stays shared by all envs.
        The plate's mass / density and the robot's body_masses are channels of the engine (set_up_domain_randomization); mass / density of any
        other rigid-prim view are refused here.
        PARITY UNPINNED: whether PhysX rescales anything on `set_local_scales` rests on that question-marked author comment (the same line
        sits in every task YAML of the reference, e.g. JointLocomanipulation.yaml:166), and the factors come from a private torch.Generator
        seeded with the config seed, not from the global stream the reference seeds with `torch.manual_seed` before
        `randomize_scale_on_startup` - `startup_scales` records this repo's draws, not the reference's.  The entry is accepted (with the
        warning) rather than refused because the reference's own YAML block has to load entry for entry (`test_reference_dr_block_loads_verbatim`);
        `sim.engine.refuse_startup_scale: true` turns the warning into a NotImplementedError for users who prefer the loud failure."""
        if not self.randomize:
            return
        import warnings
        import torch
        params = self._cfg["domain_randomization"]["randomization_params"]
        for group in ("rigid_prim_views", "articulation_views"):
            for view, attrs in (params.get(group) or {}).items():
                for attribute, entry in (attrs or {}).items():
                    if entry is None or "on_startup" not in entry or attribute == "material_properties":
                        continue          # material_properties on_startup is a channel of the engine (set_up_domain_randomization)
                    if attribute in _RESET_STATE:
                        continue          # reset-state entries: set_up_domain_randomization refuses every trigger but on_reset, with the reason
                    if attribute == "body_masses" and group == "articulation_views":
                        continue          # a mass channel of the engine (set_up_domain_randomization)
                    if attribute in _ACTUATOR and group == "articulation_views":
                        continue          # an actuator channel of the engine (set_up_domain_randomization)
                    if attribute in ("mass", "density") and group == "rigid_prim_views":
                        if view != PLATE_VIEW:
                            raise NotImplementedError(_MASS_REFUSED.format(view=view, attribute=attribute))
                        if not hasattr(task, "robot_manipulation"):
                            raise NotImplementedError(_NO_PLATE.format(view=view, attribute=attribute))
                        continue          # the plate's mass / density: mass channels of the engine too
                    st = entry["on_startup"]
                    if not set(_ON_RESET_KEYS).issubset(st.keys()):          # randomize.py:75-77,104-106
                        raise ValueError(f"Please ensure the following randomization parameters for {view} {attribute} on_startup are provided: "
                                         "operation, distribution, distribution_parameters.")
                    if attribute == "scale" and bool((self._cfg.get("sim", {}).get("engine", {}) or {}).get("refuse_startup_scale", False)):
                        raise NotImplementedError(f"{group}.{view}.scale on_startup does not enter this engine's dynamics (sim.engine.refuse_startup_scale is set)")
                    if attribute != "scale":
                        raise NotImplementedError(f"domain randomisation of {group}.{view}.{attribute} on_startup is not implemented")
                    n = int(self._cfg["env"]["numEnvs"])
                    g = torch.Generator().manual_seed(int(self._config.get("seed", 42)))
                    lo, hi = (float(x) for x in st["distribution_parameters"])
                    dist = str(st["distribution"])
                    if dist == "uniform":
                        f = lo + (hi - lo) * torch.rand(n, generator=g)
                    elif dist in ("loguniform", "log_uniform"):
                        f = torch.exp(np.log(lo) + (np.log(hi) - np.log(lo)) * torch.rand(n, generator=g))
                    elif dist in ("gaussian", "normal"):
                        f = lo + hi * torch.randn(n, generator=g)
                    else:
                        raise ValueError(f"{view} scale on_startup: unsupported distribution {dist!r}")
                    op = str(st["operation"])
                    if op not in ("scaling", "additive", "direct"):
                        raise ValueError(f"{view} scale on_startup: unsupported operation {op!r}")
                    self.startup_scales[(group, view)] = (1.0 * f) if op in ("scaling", "direct") else (1.0 + f)
                    self.active_domain_randomizations[(group, view, attribute, "on_startup")] = np.array(st["distribution_parameters"])
                    warnings.warn(f"{group}.{view}.scale on_startup: accepted; the factors ({lo}..{hi}) are drawn and kept in "
                                  "Randomizer.startup_scales but do not enter the dynamics (in the reference set_local_scales on the articulation "
                                  "root does not rescale the simulated links either)")

    def set_up_domain_randomization(self, task):
        """randomize.py:125-166: walk the YAML block; here it fills the engine's channel table."""
        if not self.randomize:
            return
        params = self._cfg["domain_randomization"]["randomization_params"]
        for opt, body in params.items():
            if opt == "observations":
                self._set_up_noise(task, "observations", body, DR_OBS_RESET, DR_OBS_INTERVAL)
                task.randomize_observations = True
                self._observations_dr_params = body
            elif opt == "actions":
                self._set_up_noise(task, "actions", body, DR_ACT_RESET, DR_ACT_INTERVAL)
                task.randomize_actions = True
                self._actions_dr_params = body
            elif opt == "simulation":
                for attribute, entry in (body or {}).items():
                    if attribute != "gravity":
                        raise NotImplementedError(f"domain randomisation of simulation.{attribute} is not implemented")
                    self._set_up_attribute(("simulation", attribute), entry, DR_GRAVITY, vector=True)
            elif opt == "rigid_prim_views":
                for view, attrs in (body or {}).items():
                    for attribute, entry in (attrs or {}).items():
                        if attribute == "scale":
                            continue          # on_startup entry, handled above
                        if attribute in ("mass", "density"):
                            if view != PLATE_VIEW:
                                raise NotImplementedError(_MASS_REFUSED.format(view=view, attribute=attribute))
                            if not hasattr(task, "robot_manipulation"):
                                raise NotImplementedError(_NO_PLATE.format(view=view, attribute=attribute))
                            self._set_up_mass(("rigid_prim_views", view, attribute), entry, DR_MASS_PLATE if attribute == "mass" else DR_MASS_PLATE_DENSITY, task)
                            continue
                        if attribute == "material_properties" and view == PLATE_VIEW:
                            self._set_up_material(("rigid_prim_views", view, attribute), entry, DR_MAT_OTHER)
                            continue
                        if attribute in ("position", "orientation") and view == PLATE_VIEW:
                            if not hasattr(task, "robot_manipulation"):
                                raise NotImplementedError(f"rigid_prim_views.{view}.{attribute}: this task has no manipulation block, so there is no plate to "
                                                          f"reset; the base's reset pose is articulation_views.<robot>.{attribute}")
                            self._set_up_reset_state(("rigid_prim_views", view, attribute), entry, (MODE_MANI,))
                            continue
                        if attribute != "force":
                            raise NotImplementedError(f"domain randomisation of rigid_prim_views.{view}.{attribute} is not implemented")
                        self._set_up_attribute(("rigid_prim_views", view, attribute), entry, DR_BASE_FORCE, vector=True)
            elif opt == "articulation_views":
                for view, attrs in (body or {}).items():
                    for attribute, entry in (attrs or {}).items():
                        if attribute == "scale":
                            continue
                        if attribute == "material_properties":          # the feet: the robot's only colliders
                            self._set_up_material(("articulation_views", view, attribute), entry, DR_MAT_ROBOT)
                            continue
                        if attribute == "body_masses":
                            self._set_up_mass(("articulation_views", view, attribute), entry, DR_MASS_BODIES, task)
                            continue
                        if attribute in _ACTUATOR:
                            self._set_up_actuator(("articulation_views", view, attribute), entry)
                            continue
                        if attribute == "joint_friction":          # the joint friction coefficient itself is not modelled: scaling it changes nothing
                            import warnings
                            warnings.warn(f"articulation_views.{view}.joint_friction: joint friction is not modelled by this engine; entry ignored")
                            continue
                        if attribute in _RESET_STATE:
                            if attribute in ("position", "orientation"):
                                if not hasattr(task, "robot_locomotion"):
                                    raise NotImplementedError(f"articulation_views.{view}.{attribute}: the robot's base is fixed in a manipulation task; the "
                                                              f"free body there is the plate (rigid_prim_views.{PLATE_VIEW}.{attribute})")
                                modes = (MODE_LOCO,)
                            else:
                                modes = (MODE_LOCO, MODE_MANI)
                            self._set_up_reset_state(("articulation_views", view, attribute), entry, modes)
                            continue
                        ch = {"max_efforts": DR_MAX_EFFORT, "joint_max_velocities": DR_MAX_VELOCITY, "damping": DR_JOINT_DAMPING}.get(attribute)
                        if ch is None:
                            raise NotImplementedError(f"domain randomisation of articulation_views.{view}.{attribute} is not implemented")
                        self._set_up_attribute(("articulation_views", view, attribute), entry, ch, vector=False)
            else:
                raise ValueError(f"unknown domain randomisation group {opt!r}")
        self._check_mass_ranges(task)

    def _set_up_noise(self, task, kind, body, ch_reset, ch_interval):
        if body is None:
            raise ValueError(f"{kind.capitalize()} randomization parameters are not provided.")          # randomize.py:170-171
        if "on_reset" in body:
            self._channels[ch_reset] = _channel(kind, body["on_reset"], "on_reset", vector=False)
            self.active_domain_randomizations[(kind, "on_reset")] = np.array(body["on_reset"]["distribution_parameters"])
        if "on_interval" in body:
            self._channels[ch_interval] = _channel(kind, body["on_interval"], "on_interval", vector=False)
            self.active_domain_randomizations[(kind, "on_interval")] = np.array(body["on_interval"]["distribution_parameters"])
        for c in (ch_reset, ch_interval):
            if self._channels[c].enabled and self._channels[c].operation == DR_OPERATIONS["direct"]:
                raise ValueError(f"{kind}: operation must be additive or scaling")

    def _set_up_attribute(self, key, entry, ch, vector):
        if entry is None:
            raise ValueError(f"Randomization parameters for {'.'.join(key)} is not provided.")
        if "on_reset" in entry and "on_interval" in entry:
            raise NotImplementedError(f"{'.'.join(key)}: give either on_reset or on_interval, not both")
        for trigger in ("on_reset", "on_interval"):
            if trigger in entry:
                self._channels[ch] = _channel(".".join(key), entry[trigger], trigger, vector)
                self.active_domain_randomizations[key + (trigger,)] = np.array(entry[trigger]["distribution_parameters"])

    def _set_up_reset_state(self, key, entry, modes):
        """joint_positions / joint_velocities / position / orientation on_reset -> the reset-state channel of the blocks of `modes`."""
        attribute = key[-1]
        ch = _reset_state_channel(".".join(key), attribute, entry)
        for m in modes:
            self._reset_channels[m][_RESET_STATE[attribute][0]] = ch
        self.active_domain_randomizations[key + ("on_reset",)] = np.array(entry["on_reset"]["distribution_parameters"])

    def _set_up_mass(self, key, entry, ch, task):
        """plate mass / density or body_masses: one trigger -> the mass channel `ch`; per-body parameters go from body_names order to table order."""
        trigger, c, lo, hi = _mass_channel(".".join(key), key[-1], entry)
        self._mass_channels[ch] = c
        if ch == DR_MASS_BODIES:
            order = self._robot_model(task).table_body_order()
            self._mass_body_p0 = [float(lo[k]) for k in order]
            self._mass_body_p1 = [float(hi[k]) for k in order]
        self.active_domain_randomizations[key + (trigger,)] = np.array(entry[trigger]["distribution_parameters"])

    def _set_up_actuator(self, key, entry):
        """joint_kps / joint_kds / command_latency: one trigger -> the actuator channel of every block (check_actuator scopes it)."""
        trigger, c = _actuator_channel(".".join(key), key[-1], entry)
        self._actuator_channels[_ACTUATOR[key[-1]]] = c
        self._actuator_where[_ACTUATOR[key[-1]]] = ".".join(key)
        self.active_domain_randomizations[key + (trigger,)] = np.array(entry[trigger]["distribution_parameters"])

    def check_actuator(self, ep):
        """The actuator entries against the block they reach (called by the task when it builds the block): the actuator family decides which
        entries exist, and a bounded gain range must stay positive for THIS block's nominal gains."""
        if not self.randomize:
            return
        ckp, ckd, cl = (self._actuator_channels[c] for c in (DR_ACTUATOR_KP, DR_ACTUATOR_KD, DR_ACTUATOR_LATENCY))
        w = self._actuator_where
        pd = int(ep.variant) >= 1
        if ckp.enabled and not pd and int(ep.drive_mode) != 1:
            raise NotImplementedError(f"{w[DR_ACTUATOR_KP]}: there is no position gain in {'effort' if int(ep.drive_mode) == 2 else 'velocity'} control "
                                      "(the drive has a velocity gain only: joint_kds); joint_kps exists on the PD-actuator tasks and in position control")
        if ckd.enabled and not pd and int(ep.drive_mode) == 2:
            raise NotImplementedError(f"{w[DR_ACTUATOR_KD]}: effort control runs with the drive gains off, so there is no velocity gain to randomise")
        if cl.enabled and not pd:
            raise NotImplementedError(f"{w[DR_ACTUATOR_LATENCY]}: the command latency exists on the PD-actuator tasks only (controller variants 1 / 2: "
                                      "the PD law is re-evaluated every sub-step there); the velocity-drive tasks have none")
        for c, name, nominal in ((ckp, "joint_kps", float(ep.pd_kp)), (ckd, "joint_kds", float(ep.kd))):
            if not c.enabled:
                continue
            least = _least_mass(c, c.p0[0], c.p1[0], nominal)
            if least is not None and least <= 0:
                raise ValueError(f"{w[_ACTUATOR[name]]}: the distribution's range reaches a non-positive gain ({least:g} on a nominal of {nominal:g}); "
                                 "a gaussian is floored instead, a uniform / loguniform range must stay positive")

    @staticmethod
    def _robot_model(task):
        from ...model.robot_model import load_model
        return load_model(getattr(task, "model_asset", "quadruped_robot_v2"))

    def _check_mass_ranges(self, task):
        """A bounded distribution whose range reaches a non-positive mass is refused (the floor is for gaussian tails only).  The density factor
        and the body masses are checked here; the plate's mass against the plate of the block it reaches (check_plate_mass_range)."""
        cd, cb = self._mass_channels[DR_MASS_PLATE_DENSITY], self._mass_channels[DR_MASS_BODIES]
        if cd.enabled:
            least = _least_mass(cd, cd.p0[0], cd.p1[0], 1.0)
            if least is not None and least <= 0:
                raise ValueError(f"rigid_prim_views.{PLATE_VIEW}.density: the distribution's range reaches a non-positive factor ({least:g})")
        if cb.enabled:
            rm = self._robot_model(task)
            for slot, k in enumerate(rm.table_body_order()):
                least = _least_mass(cb, self._mass_body_p0[slot], self._mass_body_p1[slot], float(rm.mass[k]))
                if least is not None and least <= 0:
                    raise ValueError(f"articulation_views.<robot>.body_masses: the distribution's range reaches a non-positive mass ({least:g} kg) for "
                                     f"body {rm.body_names[k]!r}; a gaussian is floored instead, a uniform / loguniform range must stay positive")

    def check_plate_mass_range(self, plate_mass: float):
        """The plate-mass entry against the nominal of the manipulation block it reaches: `plate_mass` of that block times the least density
        factor.  Called by the task when it builds the block, so a task with another plate is checked against its own."""
        cp, cd = self._mass_channels[DR_MASS_PLATE], self._mass_channels[DR_MASS_PLATE_DENSITY]
        if not (self.randomize and cp.enabled):
            return
        s_least = 1.0
        if cd.enabled:
            least = _least_mass(cd, cd.p0[0], cd.p1[0], 1.0)
            s_least = DR_MASS_FLOOR if least is None else least
        least = _least_mass(cp, cp.p0[0], cp.p1[0], s_least * float(plate_mass))
        if least is not None and least <= 0:
            raise ValueError(f"rigid_prim_views.{PLATE_VIEW}.mass: the distribution's range reaches a non-positive mass ({least:g} kg on a plate of "
                             f"{s_least * float(plate_mass):g} kg); a gaussian is floored instead, a uniform / loguniform range must stay positive")

    def _set_up_material(self, key, entry, ch):
        """material_properties of the robot (ch = DR_MAT_ROBOT) or the plate (DR_MAT_OTHER): one trigger, dynamic component into the engine."""
        where = ".".join(key)
        if entry is None:
            raise ValueError(f"Randomization parameters for {where} is not provided.")
        triggers = [t for t in ("on_startup", "on_reset", "on_interval") if t in entry]
        if len(triggers) != 1:
            raise NotImplementedError(f"{where}: give exactly one of on_startup, on_reset, on_interval")
        trigger = triggers[0]
        self._mat_channels[ch], self._mat_buckets[ch] = _material_channel(where, entry[trigger], trigger)
        self.active_domain_randomizations[key + (trigger,)] = np.array(entry[trigger]["distribution_parameters"])
        c = self._mat_channels[ch]
        mat = (self._cfg.get("sim", {}) or {}).get("default_physics_material", {}) or {}          # the feet and the plate carry the scene's default material
        nominal = (float(mat.get("static_friction", 1.0)), None, float(mat.get("restitution", 0.0)))
        unmodelled = [name for i, name in enumerate(_MAT_COMPONENTS) if i != 1 and _changes(c.operation, c.distribution, c.p0[i], c.p1[i], nominal[i])]
        if unmodelled:
            import warnings
            warnings.warn(f"{where} {trigger}: the {' and '.join(unmodelled)} component(s) are drawn for the record but not modelled by this engine "
                          "(one Coulomb coefficient, the dynamic one; no restitution); only dynamic_friction is randomised")

    # ------------------------------------------------------------------ engine side
    def engine_dr(self, mode: int = None) -> dict:
        """Fields of EngineParams describing the randomisation (all channels off when randomize is False).  `mode`: the block's task mode - the
        plate's material channel belongs to manipulation blocks only."""
        if not self.randomize:
            return dict(dr_enabled=0, dr_min_frequency=1, dr=[DRChannel() for _ in range(DR_CHANNELS)])
        mat = list(self._mat_channels); buckets = list(self._mat_buckets)
        if mode != MODE_MANI:
            mat[DR_MAT_OTHER] = DRChannel(); buckets[DR_MAT_OTHER] = 0
        mass = list(self._mass_channels)
        if mode != MODE_MANI:          # the plate's mass / density: manipulation blocks only
            mass[DR_MASS_PLATE] = DRChannel(); mass[DR_MASS_PLATE_DENSITY] = DRChannel()
        return dict(dr_enabled=1, dr_min_frequency=int(self.min_frequency), dr=list(self._channels), dr_mat=mat, dr_mat_buckets=buckets,
                    dr_reset=list(self._reset_channels[MODE_MANI if mode == MODE_MANI else MODE_LOCO]),
                    dr_mass=mass, dr_mass_body_p0=list(self._mass_body_p0), dr_mass_body_p1=list(self._mass_body_p1),
                    dr_actuator=list(self._actuator_channels))

    # The wrapper calls these two exactly where the reference does (vec_env_rlgames.py:56-58,70-72).  The noise has already been /
    # will be applied inside lm_step with the reference's counter semantics (randomize.py:212-306), so they hand the tensor through.
    def apply_actions_randomization(self, actions, reset_buf):
        return actions

    def apply_observations_randomization(self, observations, reset_buf):
        return observations
