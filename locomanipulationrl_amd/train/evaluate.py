"""Evaluation of a trained policy: what the reference's skrl scripts do with `eval = True` (load best_agent.pt, agent.set_mode('eval'),
the trainer's evaluation loop with mean actions), reported per EPISODE - how many ended, how each ended, their return and length -
rather than as the training-time window num_successes / num_resets of a sampling policy.

The fused path runs T = 48-step rollouts (include/lm_policy.h) in deterministic mode with a capped episode record attached; the
step-by-step path (`fused=False`, or an env that is not on a HIP device) is forward -> env.step(mean) -> EpisodeRecord.update, with the
torch forward on the CPU and the rollout's own forward kernel on the GPU (so the two paths of one engine walk the same trajectory).
Both apply the same record rule and return the same summary keys.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from ..lib import EpisodeRecord, TrajectoryRecord

ROLLOUT_STEPS = 48      # the reference's rollout length (scripts/skrl_ppo_locomotion.py:87)


def _scaler_moments(obs_scaler):
    if obs_scaler is None:
        return None, None, 1e-8, 5.0
    return obs_scaler.mean.float(), obs_scaler.var.float(), obs_scaler.eps, obs_scaler.clip


def evaluate(env, model, obs_scaler=None, episodes_per_env: int = 1, max_steps: Optional[int] = None, deterministic: bool = True,
             fused: bool = True, noise_seed: int = 2000, return_record: bool = False, record_envs=None, record_rows: Optional[int] = None) -> Dict:
    """Run `model` on `env` until every env has completed `episodes_per_env` episodes (the FIRST ones of every env: no bias towards short
    episodes) or `max_steps` env steps have been taken (default: episodes_per_env x the longest max_episode + one rollout).  Returns
    EpisodeRecord.summary() plus "steps", "envs_short" (envs that completed fewer episodes than asked for) and "deterministic"; with
    `return_record` also the (9, N) record itself (a host tensor) under "record".
    `record_envs` (a list of env ids) attaches a TrajectoryRecord for those envs with the same episode cap and room for `record_rows` rows per
    env (default: the task's longest max_episode x episodes_per_env); it is zeroed together with the episode record, at the reset, and
    returned under "trajectory"."""
    task = env._task
    engine = task.engine
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
    out["steps"] = steps
    out["envs_short"] = int((record.record[2] < float(cap)).sum())
    out["deterministic"] = bool(deterministic)
    if return_record:
        out["record"] = record.record.detach().cpu().clone()
    if traj is not None:
        out["trajectory"] = traj
    return out
