"""Policy evaluation, host side (no GPU): the episode-record rule against an independent numpy reference (tests/episode_reference.py) on
hand-made streams and on forced outcomes of the CPU oracle, evaluate() on the oracle backend, PPO checkpoints, the header constant and
the two boundary accessors the reference's scripts use (env.unwrapped, task.get_extras())."""
import dataclasses
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import episode_reference as er
import locomanipulationrl_amd as lm
from conftest import ROOT
from locomanipulationrl_amd import lib as lmlib
from locomanipulationrl_amd.lib import EpisodeRecord
from locomanipulationrl_amd.model.robot_model import load_model
from locomanipulationrl_amd.policies.mlp_model import SharedMLP
from locomanipulationrl_amd.train.evaluate import evaluate
from locomanipulationrl_amd.train.ppo import PPO
from oracle_backend import OracleEngine, oracle_engine_factory

F32 = np.float32


def make(task, n, **kw):
    return lm.make_env(task, num_envs=n, engine_factory=oracle_engine_factory, sim_device="cpu", rl_device="cpu", **kw)


# ---------------------------------------------------------------------------------------------- the reference on hand-made streams
def test_reference_episode_spanning_three_rollouts():
    rec = er.new_record(1)
    rew = [F32(0.1), F32(0.2), F32(0.3), F32(0.4), F32(0.5), F32(0.6), F32(0.7)]
    er.update(rec, [[rew[0]], [rew[1]], [rew[2]]], [[0], [0], [0]], [[0], [0], [0]], 300)          # "rollout" 1: nothing ends
    assert rec[er.RUN_LENGTH, 0] == 3 and rec[er.EPISODES, 0] == 0 and rec[er.RUN_RETURN, 0] == F32(F32(rew[0] + rew[1]) + rew[2])
    er.update(rec, [[rew[3]], [rew[4]]], [[0], [0]], [[0], [0]], 300)                              # rollout 2
    er.update(rec, [[rew[5]], [rew[6]]], [[1], [0]], [[1], [0]], 300)                              # rollout 3: the episode ends by goal, the next begins
    ret = F32(0)
    for r in rew[:6]:
        ret = F32(ret + r)
    assert rec[:, 0].tolist() == [rew[6], 1.0, 1.0, ret, 6.0, 1.0, 0.0, 0.0, ret]
    # the reward of the ending step belongs to the episode it ends; the step after starts from zero
    assert rec[er.LAST_RETURN, 0] == ret and rec[er.RUN_RETURN, 0] == rew[6]


def test_reference_outcomes_cap_and_two_blocks():
    M = 6
    # env 0: goal at length 3; env 1: timeout at length M - 1; env 2: failure at length 2; env 3: a failure on step M - 1 counts as a timeout
    T = 5
    dones = np.zeros((T, 4), np.int64); goals = np.zeros((T, 4), np.int64); rew = np.ones((T, 4), F32)
    dones[2, 0] = 1; goals[2, 0] = 1
    dones[4, 1] = 1
    dones[1, 2] = 1
    dones[4, 3] = 1            # (whatever made it end: at length M - 1 it is a timeout)
    rec = er.update(er.new_record(4), rew, dones, goals, M)
    assert rec[er.GOAL].tolist() == [1, 0, 0, 0] and rec[er.TIMEOUT].tolist() == [0, 1, 0, 1] and rec[er.FAILURE].tolist() == [0, 0, 1, 0]
    assert rec[er.SUM_LENGTH].tolist() == [3, 5, 2, 5] and rec[er.RUN_LENGTH].tolist() == [2, 0, 3, 0] and rec[er.LAST_RETURN].tolist() == [3, 5, 2, 5]
    # the outcome is read from the flags, not from the reward: a negative reward on a goal step is still a goal
    rec2 = er.update(er.new_record(1), [[F32(-7.0)]], [[1]], [[1]], M)
    assert er.tallies(rec2) == (1, 1, 0, 0)
    # the cap freezes an env after `cap` episodes: every later step is ignored, running rows included
    d = np.zeros((9, 2), np.int64); d[[1, 3, 5, 7], 0] = 1; d[8, 1] = 1
    rec3 = er.update(er.new_record(2), np.ones((9, 2), F32), d, np.zeros((9, 2), np.int64), 300, cap=2)
    assert rec3[:, 0].tolist() == [0, 0, 2, 4, 4, 0, 0, 2, 2] and rec3[:, 1].tolist() == [0, 0, 1, 9, 9, 0, 0, 1, 9]
    rec4 = er.update(rec3.copy(), np.ones((3, 2), F32), np.ones((3, 2), np.int64), np.zeros((3, 2), np.int64), 300, cap=2)
    assert rec4[:, 0].tolist() == rec3[:, 0].tolist() and rec4[er.EPISODES, 1] == 2 and rec4[er.SUM_LENGTH, 1] == 10
    # two blocks with different M: the same stream is a timeout in the block with M = 4 and a failure in the block with M = 300
    d = np.zeros((3, 2), np.int64); d[2] = 1
    rec5 = er.update(er.new_record(2), np.ones((3, 2), F32), d, np.zeros((3, 2), np.int64), np.array([4, 300]))
    assert rec5[er.TIMEOUT].tolist() == [1, 0] and rec5[er.FAILURE].tolist() == [0, 1]


# ---------------------------------------------------------------------------------------------- EpisodeRecord (torch path) on the CPU oracle
FORCED = [("QuadrupedPoseControl", dict(h_base=1.0), 6, er.FAILURE, 48, 1),
          ("QuadrupedPoseControl", dict(max_episode=6), 14, er.TIMEOUT, 16, 5),
          ("QuadrupedPoseControl", dict(succ_thresh=4.0, max_consec=3), 16, er.GOAL, 24, 5),
          ("QuadrupedManipulatePlate", dict(succ_thresh=4.0, max_consec=3), 16, er.GOAL, 24, 5)]


def oracle_engine(task_name, n, **changes):
    env = make(task_name, n)
    task = env._task
    params = [dataclasses.replace(p, **changes) for p in task.engine_params()]
    return OracleEngine(load_model(task.model_asset), params, n, task.split_env(), 42, 5.0, 1.0), params


@pytest.mark.parametrize("task_name,changes,steps,outcome,count,length", FORCED)
def test_episode_record_torch_path_equals_reference_on_forced_outcomes(task_name, changes, steps, outcome, count, length):
    N = 8
    eng, params = oracle_engine(task_name, N, **changes)
    record = EpisodeRecord(eng)
    rews, dones, goals = [], [], []
    for t in range(steps):
        r = torch.zeros(N); d = torch.zeros(N, dtype=torch.int64)
        eng.step(torch.zeros(N, 12), None, None, None, r, d)
        assert torch.equal(eng.terms[7] != 0, eng.cnt[2] != 0)            # the terms' goal_reset row is goal_reset_buf on every step
        record.update(r, d)
        rews.append(r.numpy().copy()); dones.append(d.numpy().copy()); goals.append(eng.terms[7].numpy().copy())
    ref = er.update(er.new_record(N), np.stack(rews), np.stack(dones), np.stack(goals), params[0].max_episode)
    episodes = int(ref[er.EPISODES].sum())
    assert episodes > 0 and ref[outcome].sum() >= 0.9 * episodes, er.tallies(ref)          # the reference's own tallies first
    assert int(ref[outcome].sum()) == count and float(ref[er.SUM_LENGTH].sum()) == length * count
    assert np.array_equal(record.record.numpy(), ref)                                      # exact: plain fp32 adds in step order
    s = record.summary()
    assert s["episodes"] == episodes and s[{er.GOAL: "success_rate", er.TIMEOUT: "timeout_rate", er.FAILURE: "failure_rate"}[outcome]] == 1.0
    assert s["mean_length"] == length and abs(s["mean_return"] - ref[er.SUM_RETURN].astype(np.float64).sum() / episodes) < 1e-12


def test_episode_record_torch_path_cap_and_two_blocks():
    """A co-training engine whose blocks have different max_episode, with a cap: every env stops at `cap` episodes."""
    env = make("JointLocomanipulation", 32)
    task = env._task
    p = task.engine_params()
    params = [dataclasses.replace(p[0], max_episode=6), dataclasses.replace(p[1], max_episode=4)]
    eng = OracleEngine(load_model(task.model_asset), params, 32, task.split_env(), 42, 5.0, 1.0)
    record = EpisodeRecord(eng)
    assert record.split == task.split_env() == 16
    rews, dones, goals = [], [], []
    for t in range(12):
        r = torch.zeros(32); d = torch.zeros(32, dtype=torch.int64)
        eng.step(torch.zeros(32, 12), None, None, None, r, d)
        record.update(r, d, 2)
        rews.append(r.numpy().copy()); dones.append(d.numpy().copy()); goals.append(eng.terms[7].numpy().copy())
    M = np.array([6] * 16 + [4] * 16)
    ref = er.update(er.new_record(32), np.stack(rews), np.stack(dones), np.stack(goals), M, cap=2)
    assert (ref[er.EPISODES] == 2).all() and (ref[er.TIMEOUT] == 2).all()
    assert ref[er.SUM_LENGTH, :16].tolist() == [10.0] * 16 and ref[er.SUM_LENGTH, 16:].tolist() == [6.0] * 16
    assert np.array_equal(record.record.numpy(), ref)
    s = record.summary()
    assert s["episodes"] == 64 and s["loco"]["mean_length"] == 5.0 and s["mani"]["mean_length"] == 3.0 and s["loco"]["timeout_rate"] == 1.0


# ---------------------------------------------------------------------------------------------- evaluate() on the oracle backend
@pytest.mark.parametrize("deterministic", [True, False])
def test_evaluate_step_by_step_on_the_oracle_backend(deterministic):
    torch.manual_seed(0)
    N, per_env = 8, 2
    env = make("QuadrupedPoseControl", N, overrides={"task": {"sim": {"max_episode_length": 6}}})
    assert env._task.engine_params()[0].max_episode == 6
    out = evaluate(env, SharedMLP(), None, episodes_per_env=per_env, deterministic=deterministic, fused=False)
    for k in ("episodes", "mean_return", "mean_length", "success_rate", "timeout_rate", "failure_rate", "steps", "envs_short"):
        assert k in out, k
    assert out["episodes"] == N * per_env and out["envs_short"] == 0 and out["steps"] <= per_env * 6
    assert abs(out["success_rate"] + out["timeout_rate"] + out["failure_rate"] - 1.0) < 1e-12
    assert 1.0 <= out["mean_length"] <= 5.0 and np.isfinite(out["mean_return"])
    # a step budget that is too small is reported, not hidden
    env2 = make("QuadrupedPoseControl", N, overrides={"task": {"sim": {"max_episode_length": 6}}})
    short = evaluate(env2, SharedMLP(), None, episodes_per_env=50, max_steps=7, deterministic=True, fused=False)
    assert short["steps"] == 7 and short["envs_short"] == N and short["episodes"] < 50 * N


# ---------------------------------------------------------------------------------------------- checkpoints
def _same(a, b):
    if isinstance(a, torch.Tensor):
        return torch.equal(a.cpu(), b.cpu())
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def test_ppo_checkpoint_round_trip_and_identical_next_update(tmp_path):
    torch.manual_seed(0)
    env = make("QuadrupedPoseControl", 16)
    a = PPO(env, SharedMLP(), rollouts=4, learning_epochs=2, hip_inference=False)
    a.train(8, log_every=1, log=lambda r: None)          # two iterations: the scalers, the KL-adaptive lr and Adam's moments have moved
    path = str(tmp_path / "agent.pt")
    a.save(path)
    torch.manual_seed(123)
    b = PPO(env, SharedMLP(), rollouts=4, learning_epochs=2, hip_inference=False)
    assert not _same(a.model.state_dict(), b.model.state_dict())
    b.load(path)
    assert _same(a.model.state_dict(), b.model.state_dict())
    for name in ("obs_scaler", "val_scaler"):
        sa, sb = getattr(a, name), getattr(b, name)
        assert torch.equal(sa.mean, sb.mean) and torch.equal(sa.var, sb.var) and torch.equal(sa.count, sb.count) and sb.mean.dtype == torch.float64
    assert a.lr == b.lr and all(g["lr"] == a.lr for g in b.opt.param_groups) and _same(a.opt.state_dict(), b.opt.state_dict())
    assert int(a.obs_scaler.count) > 1 and len(a.opt.state_dict()["state"]) > 0
    # one further update on identical buffers: bit-equal parameters on both
    for name in ("b_obs", "b_act", "b_logp", "b_val", "b_rew", "b_done"):
        getattr(b, name).copy_(getattr(a, name))
    last = torch.zeros(16)
    a.update(last); b.update(last)
    assert _same(a.model.state_dict(), b.model.state_dict()) and a.lr == b.lr


# ---------------------------------------------------------------------------------------------- header and layout
def test_episode_rows_constant_and_unchanged_abi():
    src = '#include <stdio.h>\n#include "lm_engine.h"\n#include "lm_policy.h"\nint main(){printf("%d %d %zu\\n", LM_EPISODE_ROWS, LM_ABI_VERSION, sizeof(lm_params));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c"); open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        rows, abi, size = map(int, subprocess.check_output([exe]).split())
    assert rows == lmlib.EPISODE_ROWS == er.ROWS == 9 and len(lmlib.EPISODE) == rows
    assert abi == lmlib.ABI_VERSION == 5 and size == lmlib.C.sizeof(lmlib.LmParams) == 1404
    so = (lmlib.build_library(), lmlib.load_library())[1]
    # the LM_EINVAL cases that need no device
    assert so.lm_rollout_set_deterministic(None, 1) == -1 and b"lm_rollout_set_deterministic" in so.lm_last_error()
    assert so.lm_rollout_set_episode_record(None, None, 0) == -1 and b"lm_rollout_set_episode_record" in so.lm_last_error()
    assert so.lm_episode_update(None, None, None, None, 0, None) == -1 and b"lm_episode_update" in so.lm_last_error()
    hdr = open(os.path.join(ROOT, "include", "lm_policy.h")).read()
    assert re.search(r"counts as a timeout", hdr) and re.search(r"exact below 2\^24", hdr)


# ---------------------------------------------------------------------------------------------- boundary
def test_unwrapped_and_get_extras():
    env = make("QuadrupedPoseControl", 16)
    assert env.unwrapped is env
    env.reset()
    env.step(torch.zeros(16, 12))
    task = env.unwrapped._task
    assert task.get_extras() is task.extras and len(task.extras) > 0
    for k in task.extras:
        assert isinstance(float(env.unwrapped._task.extras[k].item()), float)
