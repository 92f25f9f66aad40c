"""Evaluation of a trained policy: what the reference's skrl scripts do with `eval = True` (load best_agent.pt, agent.set_mode('eval'),
the trainer's evaluation loop with mean actions), reported per EPISODE - how many ended, how each ended, their return and length -
rather than as the training-time window num_successes / num_resets of a sampling policy.

The fused path runs T = 48-step rollouts (include/lm_policy.h) in deterministic mode with a capped episode record attached; the
step-by-step path (`fused=False`, or an env that is not on a HIP device) is forward -> env.step(mean) -> EpisodeRecord.update, with the
torch forward on the CPU and the rollout's own forward kernel on the GPU (so the two paths of one engine walk the same trajectory).
Both apply the same record rule and return the same summary keys.
"""
from __future__ import annotations

import itertools
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..lib import EpisodeRecord, TrajectoryRecord

ROLLOUT_STEPS = 48      # the reference's rollout length (scripts/skrl_ppo_locomotion.py:87)


def _scaler_moments(obs_scaler):
    if obs_scaler is None:
        return None, None, 1e-8, 5.0
    return obs_scaler.mean.float(), obs_scaler.var.float(), obs_scaler.eps, obs_scaler.clip


# ---- evaluation sweeps over held per-env parameters (host code; tools/eval_policy.py --sweep NAME=LO:HI:K)
SWEEP_NAMES = ("mu", "body_mass_scale", "base_mass_add", "plate_mass", "kp_scale", "kd_scale", "latency", "max_effort")


def parse_sweep(spec: str) -> Tuple[str, np.ndarray]:
    """'NAME=LO:HI:K' -> (NAME, the K values linspace(LO, HI, K); latency rounded to whole sub-steps).  ValueError for anything else."""
    try:
        name, rng = spec.split("=")
        lo, hi, k = rng.split(":")
        lo, hi, k = float(lo), float(hi), int(k)
    except ValueError:
        raise ValueError(f"sweep {spec!r}: NAME=LO:HI:K is needed (K values from LO to HI)") from None
    if name not in SWEEP_NAMES:
        raise ValueError(f"sweep {spec!r}: NAME must be one of {', '.join(SWEEP_NAMES)}")
    if k < 1 or not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError(f"sweep {spec!r}: K >= 1 and finite bounds are needed")
    v = np.linspace(lo, hi, k)
    return name, (np.round(v) if name == "latency" else v)


def sweep_grid(sweeps: Sequence[Tuple[str, np.ndarray]]) -> List[Dict[str, float]]:
    """The Cartesian product of the parsed sweeps (the last one varies fastest): one {name: value} per grid point."""
    names = [n for n, _ in sweeps]
    if len(set(names)) != len(names):
        raise ValueError(f"sweeps: {names} names a parameter twice")
    return [dict(zip(names, (float(x) for x in combo))) for combo in itertools.product(*[v for _, v in sweeps])]


def sweep_groups(num_envs: int, num_points: int) -> np.ndarray:
    """Env e evaluates grid point e % num_points: both halves of a co-training engine cover the grid (split_env is a multiple of 16, so
    choose num_envs so that each half holds whole periods if equal counts matter)."""
    if num_points < 1 or num_points > num_envs:
        raise ValueError(f"a grid of {num_points} points does not fit {num_envs} envs")
    return np.arange(int(num_envs), dtype=np.int64) % int(num_points)


def sweep_env_params(points: Sequence[Dict[str, float]], groups: np.ndarray, body_masses=None, kp=None, kd=None) -> Dict[str, np.ndarray]:
    """What Engine.set_env_params takes for the grid: per env the value of its point.  The nominal values the relative sweeps scale - the 21
    body masses in table order, per-env kp and kd - are handed in (sweep_nominals reads them from a task)."""
    N = len(groups)
    col = lambda name: np.asarray([points[g][name] for g in groups], dtype=np.float64)
    names = set(points[0]) if points else set()
    out: Dict[str, np.ndarray] = {}
    if "mu" in names: out["mu"] = col("mu")
    if "plate_mass" in names: out["plate_mass"] = col("plate_mass")
    if "latency" in names: out["latency"] = col("latency")
    if "max_effort" in names: out["max_efforts"] = np.tile(col("max_effort"), (12, 1))
    if "kp_scale" in names: out["kp"] = np.asarray(kp, dtype=np.float64) * col("kp_scale")
    if "kd_scale" in names: out["kd"] = np.asarray(kd, dtype=np.float64) * col("kd_scale")
    if names & {"body_mass_scale", "base_mass_add"}:
        m = np.repeat(np.asarray(body_masses, dtype=np.float64)[:, None], N, axis=1)
        if "body_mass_scale" in names: m = m * col("body_mass_scale")[None, :]
        if "base_mass_add" in names: m[0] = m[0] + col("base_mass_add")      # a payload on the base link (body 0 of the table order: the hub)
        out["body_masses"] = m
    return {k: v.astype(np.float32) for k, v in out.items()}


def sweep_nominals(task) -> Dict[str, np.ndarray]:
    """body_masses (21,) in table order and per-env kp / kd (N,) of a task's engine: the nominal values of the relative sweeps."""
    from ..model.robot_model import load_model
    rm = load_model(task.model_asset)
    params = task.engine_params(); N = int(task.num_envs); split = task.split_env() if len(params) == 2 else None
    per_env = lambda f: np.asarray([f(params[1 if (split and e >= split) else 0]) for e in range(N)], dtype=np.float64)
    return dict(body_masses=np.asarray([rm.mass[i] for i in rm.table_body_order()], dtype=np.float64),
                kp=per_env(lambda p: p.pd_kp), kd=per_env(lambda p: p.kd))


def evaluate(env, model, obs_scaler=None, episodes_per_env: int = 1, max_steps: Optional[int] = None, deterministic: bool = True,
             fused: bool = True, noise_seed: int = 2000, return_record: bool = False, record_envs=None, record_rows: Optional[int] = None,
             env_params: Optional[Dict] = None, groups=None) -> Dict:
    """Run `model` on `env` until every env has completed `episodes_per_env` episodes (the FIRST ones of every env: no bias towards short
    episodes) or `max_steps` env steps have been taken (default: episodes_per_env x the longest max_episode + one rollout).  Returns
    EpisodeRecord.summary() plus "steps", "envs_short" (envs that completed fewer episodes than asked for) and "deterministic"; with
    `return_record` also the (9, N) record itself (a host tensor) under "record".
    `record_envs` (a list of env ids) attaches a TrajectoryRecord for those envs with the same episode cap and room for `record_rows` rows per
    env (default: the task's longest max_episode x episodes_per_env); it is zeroed together with the episode record, at the reset, and
    returned under "trajectory".
    `env_params` (a dict for Engine.set_env_params; the task needs sim.engine.env_params) is held from before the reset on; `groups`, an int
    (N,) tensor / array of group ids, adds "groups": {id: the same summary over the envs of that group} (EpisodeRecord.summary_by)."""
    task = env._task
    engine = task.engine
    if env_params:
        task.set_env_params(**env_params)
    cap = int(episodes_per_env)
    assert cap >= 1
    if max_steps is None:
        max_steps = cap * max(int(p.max_episode) for p in task.engine_params()) + ROLLOUT_STEPS
    record = EpisodeRecord(engine)
    traj = None
    if record_envs is not None:
        rows = int(record_rows) if record_rows is not None else cap * max(int(p.max_episode) for p in task.engine_params())
        traj = TrajectoryRecord(engine, record_envs, rows, episode_cap=cap)
    # env.reset() by hand, so that the record sees the reset step too: an episode's length counts it (progress_buf is 1 after it), and the
    # timeout / failure split compares the recorded length with max_episode
    task.reset()
    o, rew, resets, _ = env.step(torch.zeros((env.num_envs, task.num_actions), device=task.rl_device))
    record.update(rew.contiguous(), resets.contiguous(), cap)
    if traj is not None:
        traj.update(rew.contiguous(), resets.contiguous())
    obs = o["obs"]
    mean_, var_, eps, clip = _scaler_moments(obs_scaler)
    on_gpu = record.record.is_cuda
    steps = 0

    def done():
        return bool((record.record[2] >= float(cap)).all())

    if fused and on_gpu:
        kind = "gnn" if type(model).__name__ == "GraphPolicy" else "mlp"
        model.refresh(engine.device, mean_, var_, eps, clip)
        packed = model._packed.clone(); log_std = model.log_std_parameter.detach().clone().float().contiguous()
        ro = task.make_rollout(kind, packed, log_std, ROLLOUT_STEPS, noise_seed=noise_seed, deterministic=deterministic,
                               episode_record=record, episode_cap=cap, trajectory_record=traj)
        ro.obs[0].copy_(obs)
        while steps < max_steps and not done():
            ro.run("auto")
            ro.obs[0].copy_(ro.obs[ROLLOUT_STEPS])
            steps += ROLLOUT_STEPS
        ro.close()
    else:
        dev = next(model.parameters()).device
        hip = on_gpu and hasattr(model, "act_inference")      # on the GPU the forward is the rollout's own kernel: both paths then compute the same bits
        if hip:
            model.refresh(engine.device, mean_, var_, eps, clip)
        with torch.no_grad():
            while steps < max_steps and not done():
                if hip:
                    mean, log_std, _ = model.act_inference(obs.contiguous())
                else:
                    x = obs.to(dev)
                    mean, log_std, _ = model(obs_scaler(x) if obs_scaler is not None else x)
                act = mean if deterministic else mean + log_std.exp() * torch.randn_like(mean)
                o, rew, resets, _ = env.step(act)
                record.update(rew.contiguous(), resets.contiguous(), cap)
                if traj is not None:
                    traj.update(rew.contiguous(), resets.contiguous())
                obs = o["obs"]; steps += 1
    out = record.summary()
    if groups is not None:
        out["groups"] = record.summary_by(groups)
    out["steps"] = steps
    out["envs_short"] = int((record.record[2] < float(cap)).sum())
    out["deterministic"] = bool(deterministic)
    if return_record:
        out["record"] = record.record.detach().cpu().clone()
    if traj is not None:
        out["trajectory"] = traj
    return out
