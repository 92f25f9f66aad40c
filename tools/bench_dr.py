"""Cost of domain randomisation inside the step launch: k_step vs k_step_dr (YAML block of QuadrupedPoseControl.yaml) at 4096 envs, and what
the contact-material channel adds to k_step_dr (the same block + the feet's material_properties, redrawn every step in 64 buckets), and what
the four reset-state channels add (the same block + joint_positions / joint_velocities / position / orientation at the reference's amplitudes,
min_frequency 0: every reset draws; and behind the YAML's min_frequency, which outlasts the run: no reset draws), and what the mass channels add
(the same block + body_masses drawn once per env / redrawn every step; on QuadrupedManipulatePlate the same pair for the plate's mass, against that
task's own randomised leg), and what the actuator channels add (joint_kps + joint_kds + command_latency on QuadrupedPoseControlCustomController,
drawn once per env / redrawn every step, against that task's own randomised leg; joint_kds alone on QuadrupedPoseControl).  Leg names given on
the command line restrict the run to those legs (ratios are printed for the pairs that ran).  `resets_per_step` is the mean number of envs
reset per timed step of each leg.
The leg `env_params` is a comparison of its own: the randomised task beside the same task with env params enabled and nothing held
(k_step_dr against k_step_dr_hp) and with every row its block reads held at what the first step recorded - three engines in one process, timed in turn,
200 steps a turn, 24 turns each; median and quartiles of the turns under "env_params"."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import locomanipulationrl_amd as lm

res = {}
MATERIAL = {"articulation_views": {"robot_view": {"material_properties": {"on_interval": dict(
    frequency_interval=1, operation="scaling", distribution="uniform", distribution_parameters=[[1.0, 0.6, 1.0], [1.0, 1.4, 1.0]], num_buckets=64)}}}}
_R = lambda prm: {"on_reset": dict(operation="additive", distribution="uniform", distribution_parameters=prm)}
RESET_STATE = {"articulation_views": {"robot_view": {"joint_positions": _R([-0.1, 0.1]), "joint_velocities": _R([-0.1, 0.1]),
                                                     "position": _R([[-0.05, -0.05, 0.0], [0.05, 0.05, 0.1]]), "orientation": _R([[-0.1, -0.1, -1.2], [0.1, 0.1, 1.2]])}}}
_M = lambda trigger, **kw: {trigger: dict(operation="scaling", distribution="uniform", distribution_parameters=[0.5, 2.0], **kw)}
BODY_MASSES = lambda e: {"articulation_views": {"robot_view": {"body_masses": e}}}
PLATE_MASS = lambda e: {"rigid_prim_views": {"plate": {"mass": e}}}
_DR = lambda prm=None, **kw: {"task": {"domain_randomization": dict(randomize=True, **({"randomization_params": prm} if prm else {}), **kw)}}
MANI = "QuadrupedManipulatePlate"
CC = "QuadrupedPoseControlCustomController"
_G = lambda trigger, **kw: {trigger: dict(operation="scaling", distribution="loguniform", distribution_parameters=[0.5, 2.0], **kw)}
_L = lambda trigger, **kw: {trigger: dict(operation="direct", distribution="uniform", distribution_parameters=[0.0, 6.0], **kw)}
ACTUATOR = lambda t, **kw: {"articulation_views": {"robot_view": {"joint_kps": _G(t, **kw), "joint_kds": _G(t, **kw), "command_latency": _L(t, **kw)}}}
JOINT_KDS = lambda e: {"articulation_views": {"robot_view": {"joint_kds": e}}}
only = set(sys.argv[1:])
resets = {}


def env_params_legs(turns=24, steps=200, N=4096):
    import numpy as np
    RAND = {"domain_randomization": {"randomize": True}}
    legs = {"randomised": {"task": RAND}, "env_params_nothing_held": {"task": {**RAND, "sim": {"engine": {"env_params": True}}}},
            "env_params_all_held": {"task": {**RAND, "sim": {"engine": {"env_params": True}}}}}
    envs = {k: lm.make_env("QuadrupedPoseControl", num_envs=N, overrides=ov) for k, ov in legs.items()}
    g = torch.Generator(device="cuda").manual_seed(0)
    pool = [torch.rand(N, 12, device="cuda", generator=g) * 2 - 1 for _ in range(16)]
    o = (torch.empty(N, 64, device="cuda"), torch.empty(N, 93, device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, dtype=torch.int64, device="cuda"), torch.empty(13, device="cuda"))
    for k, env in envs.items():
        e = env._task.engine
        for t in range(50): e.step(pool[t % 16], None, *o)
        torch.cuda.synchronize()
        if k == "env_params_all_held":
            e.set_env_params(max_efforts=e.dr_phys[0:12], max_velocities=e.dr_phys[12:24], gravity=e.dr_phys[24:27], base_force=e.dr_phys[27:30],
                             joint_damping=e.dr_phys[30:42], mu=e.dr_mu, body_masses=e.dr_body_masses, kd=e.dr_kd)
    us = {k: [] for k in envs}
    for turn in range(turns):
        for k, env in envs.items():
            e = env._task.engine
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for t in range(steps): e.step(pool[t % 16], None, *o)
            torch.cuda.synchronize(); us[k].append((time.perf_counter() - t0) / steps * 1e6)
    held = len(envs["env_params_all_held"]._task.engine.env_params_mask().nonzero()[0])
    for env in envs.values(): env.close()
    q = lambda v: dict(zip(("q1", "median", "q3"), (float(x) for x in np.percentile(v, [25, 50, 75]))))
    out = {k: q(v) for k, v in us.items()}
    out.update(turns=turns, steps_per_turn=steps, num_envs=N, rows_held=held,
               nothing_held_overhead=out["env_params_nothing_held"]["median"] / out["randomised"]["median"] - 1,
               all_held_overhead=out["env_params_all_held"]["median"] / out["randomised"]["median"] - 1)
    return out


env_params = env_params_legs() if (not only or "env_params" in only) else None
for name, ov in (("plain", None), ("randomised", {"task": {"domain_randomization": {"randomize": True}}}),
                 ("randomised_material", {"task": {"domain_randomization": {"randomize": True, "randomization_params": MATERIAL}}}),
                 ("randomised_min_frequency_0", {"task": {"domain_randomization": {"randomize": True, "min_frequency": 0}}}),
                 ("randomised_reset_state", {"task": {"domain_randomization": {"randomize": True, "min_frequency": 0, "randomization_params": RESET_STATE}}}),
                 # the same channels behind a gate that never opens (the YAML's min_frequency outlasts the run): what they cost the steps that do not draw
                 ("randomised_reset_state_gate_closed", {"task": {"domain_randomization": {"randomize": True, "randomization_params": RESET_STATE}}}),
                 # mass channels: 21 draws per env once (on_startup: the hash runs every step, the key never changes) / redrawn every step
                 ("randomised_body_masses_startup", _DR(BODY_MASSES(_M("on_startup")))),
                 ("randomised_body_masses_every_step", _DR(BODY_MASSES(_M("on_interval", frequency_interval=1)))),
                 ("mani_randomised", _DR()), ("mani_randomised_plate_mass_startup", _DR(PLATE_MASS(_M("on_startup")))),
                 ("mani_randomised_plate_mass_every_step", _DR(PLATE_MASS(_M("on_interval", frequency_interval=1)))),
                 # actuator channels: kp + kd + command latency on the custom-controller task (its own randomised leg: the YAML's block is empty,
                 # an empty joint_friction entry switches the randomised kernel on), and the velocity gain alone on the velocity drive
                 ("cc_randomised", _DR({"articulation_views": {"robot_view": {"joint_friction": {}}}})),
                 ("cc_randomised_actuator_startup", _DR(ACTUATOR("on_startup"))),
                 ("cc_randomised_actuator_every_step", _DR(ACTUATOR("on_interval", frequency_interval=1))),
                 ("randomised_joint_kds_every_step", _DR(JOINT_KDS(_G("on_interval", frequency_interval=1))))):
    if only and name not in only:
        continue
    env = lm.make_env(MANI if name.startswith("mani_") else CC if name.startswith("cc_") else "QuadrupedPoseControl", num_envs=4096, overrides=ov)
    e = env._task.engine; N = 4096
    g = torch.Generator(device="cuda").manual_seed(0)
    pool = [torch.rand(N, 12, device="cuda", generator=g) * 2 - 1 for _ in range(16)]
    o = (torch.empty(N, e.num_obs, device="cuda"), torch.empty(N, 93, device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, dtype=torch.int64, device="cuda"), torch.empty(13, device="cuda"))
    for t in range(50): e.step(pool[t % 16], None, *o)
    torch.cuda.synchronize(); ep0 = int(e.cnt[5].sum().item()); t0 = time.perf_counter()
    for t in range(500): e.step(pool[t % 16], None, *o)
    torch.cuda.synchronize(); res[name] = (time.perf_counter() - t0) / 500 * 1e6
    resets[name] = (int(e.cnt[5].sum().item()) - ep0) / 500
    env.close()
ratio = lambda a, b: res[a] / res[b] - 1 if a in res and b in res else None
print(json.dumps({"us_per_step": res, "overhead": ratio("randomised", "plain"),
                  "material_overhead_on_k_step_dr": ratio("randomised_material", "randomised"),
                  "reset_state_overhead_on_k_step_dr": ratio("randomised_reset_state", "randomised_min_frequency_0"),
                  "reset_state_gate_closed_overhead_on_k_step_dr": ratio("randomised_reset_state_gate_closed", "randomised"),
                  "body_masses_startup_overhead_on_k_step_dr": ratio("randomised_body_masses_startup", "randomised"),
                  "body_masses_every_step_overhead_on_k_step_dr": ratio("randomised_body_masses_every_step", "randomised"),
                  "plate_mass_startup_overhead_on_k_step_dr": ratio("mani_randomised_plate_mass_startup", "mani_randomised"),
                  "plate_mass_every_step_overhead_on_k_step_dr": ratio("mani_randomised_plate_mass_every_step", "mani_randomised"),
                  "actuator_startup_overhead_on_k_step_dr_pd": ratio("cc_randomised_actuator_startup", "cc_randomised"),
                  "actuator_every_step_overhead_on_k_step_dr_pd": ratio("cc_randomised_actuator_every_step", "cc_randomised"),
                  "joint_kds_every_step_overhead_on_k_step_dr": ratio("randomised_joint_kds_every_step", "randomised"),
                  "env_params": env_params, "resets_per_step": resets}))
