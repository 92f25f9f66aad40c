"""Trajectory record, host side (no GPU): the torch path of lib.TrajectoryRecord.update on the CPU oracle backend against the independent
numpy reference (tests/trajectory_reference.py) - exact equality, the record is a copy - the cap, the row limit, zero(), the files
save_npy writes, the argument errors of the Python class, and the header's constants and device-free LM_EINVAL cases."""
import dataclasses
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import trajectory_reference as tr
import locomanipulationrl_amd as lm
from conftest import ROOT
from locomanipulationrl_amd import lib as lmlib
from locomanipulationrl_amd.lib import EpisodeRecord, TrajectoryRecord
from locomanipulationrl_amd.model.robot_model import load_model
from oracle_backend import OracleEngine, oracle_engine_factory

N = 32
STEPS = 13          # max_episode 6: an episode every 5 steps, so two end inside the loop and a third is under way
# task, tracked envs (the co-training task: slots on both sides of the split at env 16), which of them sit in a manipulation block
TASKS = [("QuadrupedPoseControl", [0, 7, 31], [False, False, False]),
         ("QuadrupedManipulatePlate", [0, 7, 31], [True, True, True]),
         ("JointLocomanipulation", [0, 15, 16, 31], [False, False, True, True])]


def oracle_engine(task_name, **changes):
    env = lm.make_env(task_name, num_envs=N, engine_factory=oracle_engine_factory, sim_device="cpu", rl_device="cpu")
    task = env._task
    params = [dataclasses.replace(p, **changes) for p in task.engine_params()]
    return OracleEngine(load_model(task.model_asset), params, N, task.split_env(), 42, 5.0, 1.0), params


def walk(eng, records, steps, seed=0, observers=()):
    """`steps` steps with random actions; every record is updated after each one.  Yields (rewards, dones) after the updates."""
    g = torch.Generator().manual_seed(seed)
    for t in range(steps):
        r = torch.zeros(N); d = torch.zeros(N, dtype=torch.int64)
        eng.step(torch.rand(N, 12, generator=g) * 2.0 - 1.0, None, None, None, r, d)
        for rec in records:
            rec.update(r, d)
        for ob in observers:
            ob(r, d)
        yield r, d


@pytest.fixture(scope="module")
def walks():
    """One walk per task, shared by the tests below and left unchanged: cap 1, cap 0 and a short record side by side with the reference and
    an episode record."""
    out = {}
    for task_name, ids, mani in TASKS:
        eng, params = oracle_engine(task_name, max_episode=6)
        first = TrajectoryRecord(eng, ids, 2 * STEPS, episode_cap=1)
        every = TrajectoryRecord(eng, ids, 2 * STEPS, episode_cap=0)
        short = TrajectoryRecord(eng, ids, 3, episode_cap=0)
        epi = EpisodeRecord(eng)
        refs = {name: tr.new_record(len(ids), rec.max_rows) for name, rec in (("first", first), ("every", every), ("short", short))}
        caps = {"first": 1, "every": 0, "short": 0}
        guard = torch.full((1, 3, 64), 12345.0)          # the torch path must not reach past a slot either: rows + one guard slot in one tensor
        whole = torch.cat([short.rows, guard]); short.rows = whole[:len(ids)]
        dones = []
        for r, d in walk(eng, [first, every, short], STEPS, observers=[lambda r, d: epi.update(r, d, 1)]):
            for name, (rows, hdr) in refs.items():
                tr.update(rows, hdr, eng.state.numpy(), eng.cnt.numpy(), r.numpy(), d.numpy(), ids, mani, cap=caps[name])
            dones.append(d.numpy().copy())
        out[task_name] = dict(eng=eng, ids=ids, mani=mani, first=first, every=every, short=short, epi=epi, refs=refs, dones=np.stack(dones), guard=whole[len(ids):])
    return out


@pytest.mark.parametrize("task_name", [t[0] for t in TASKS])
def test_torch_path_equals_reference(walks, task_name):
    w = walks[task_name]
    ends = w["dones"][:, w["ids"]].sum(0)
    assert (ends >= 2).all(), ends                                    # at least two episodes of every tracked env end inside the loop
    for name in ("first", "every", "short"):
        rows, hdr = w["refs"][name]
        assert np.array_equal(w[name].header.numpy(), hdr), (name, w[name].header, hdr)
        assert tr.same_bits(w[name].rows.numpy(), rows), name
    # the free body is the base on the locomotion side and the plate on the manipulation side
    eng = w["eng"]
    for k, (e, m) in enumerate(zip(w["ids"], w["mani"])):
        last = w["every"].rows[k, STEPS - 1]
        assert torch.equal(last[24:31], eng.state[37:44, e] if m else eng.state[0:7, e])
        assert torch.equal(last[0:12], eng.state[13:25, e]) and float(last[62]) == float(eng.cnt[4, e])


@pytest.mark.parametrize("task_name", [t[0] for t in TASKS])
def test_cap_row_limit_and_zero(walks, task_name):
    w = walks[task_name]
    first, every, short = w["first"], w["every"], w["short"]
    for k, e in enumerate(w["ids"]):
        ends = np.nonzero(w["dones"][:, e])[0]
        L = int(ends[0]) + 1
        # cap 1 stops at the terminal row, inclusive: L rows, the last one flagged done, nothing behind it
        assert first.header[k].tolist() == [L, 1, 0, 0]
        assert float(first.rows[k, L - 1, 60]) == 1.0 and not first.rows[k, :L - 1, 60].any() and not first.rows[k, L:].any()
        # cap 0 keeps going: every step is a row, every end is counted
        assert every.header[k].tolist() == [STEPS, len(ends), 0, 0]
        assert torch.equal(every.rows[k, :L], first.rows[k, :L])
        # three rows of room: the rest is counted as dropped, and episodes are still counted
        assert short.header[k].tolist() == [3, len(ends), STEPS - 3, 0]
        assert torch.equal(short.rows[k], every.rows[k, :3])
    assert bool((w["guard"] == 12345.0).all())
    # zero() restarts (on copies: the shared walk stays as it is)
    eng2, _ = oracle_engine(task_name, max_episode=6)
    rec = TrajectoryRecord(eng2, w["ids"], 4, episode_cap=1)
    for _ in walk(eng2, [rec], 2):
        pass
    assert rec.header[:, 0].tolist() == [2] * len(w["ids"]) and rec.rows[:, :2].abs().sum() > 0
    rec.zero()
    assert not rec.rows.any() and not rec.header.any()
    for _ in walk(eng2, [rec], 1, seed=1):
        pass
    assert rec.header[:, 0].tolist() == [1] * len(w["ids"])
    assert float(rec.rows[0, 0, 62]) == float(eng2.cnt[4, w["ids"][0]]) > 0 and not rec.rows[:, 1:].any()          # the third step stands in row 0


@pytest.mark.parametrize("task_name", [t[0] for t in TASKS])
def test_episodes_and_save_npy(walks, task_name, tmp_path):
    w = walks[task_name]
    first, every, short, epi = w["first"], w["every"], w["short"], w["epi"]
    paths = first.save_npy(str(tmp_path), "traj")
    assert [os.path.basename(p) for p in paths] == [f"traj_env{e}.npy" for e in w["ids"]]
    for k, (e, path) in enumerate(zip(w["ids"], paths)):
        q = np.load(path)
        L = int(epi.record[4, e])                                      # the length of the first episode by the episode record (cap 1) run alongside
        assert q.dtype == np.float32 and q.shape == (L, 12) and int(epi.record[2, e]) == 1
        eps = first.episodes(k)
        assert len(eps) == 1 and eps[0]["complete"] and not eps[0]["truncated"]
        assert tr.same_bits(q, first.rows[k, :L, 0:12].numpy()) and tr.same_bits(q, eps[0]["q"])
        z = np.load(path[:-4] + ".npz")
        assert z["header"].tolist() == first.header[k].tolist() and int(z["env"]) == e and int(z["episodes"]) == 1
        for name, sl in TrajectoryRecord.COLUMNS.items():
            want = first.rows[k, :L, sl].numpy()
            assert tr.same_bits(z[f"{name}_0"].reshape(L, -1), want), name
    # every episode of an uncapped record, cut at the done flags; a short record is marked truncated
    paths = every.save_npy(str(tmp_path), "all")
    for k, e in enumerate(w["ids"]):
        ends = np.nonzero(w["dones"][:, e])[0]
        eps = every.episodes(k)
        bounds = [0] + [int(i) + 1 for i in ends]
        assert [len(ep["reward"]) for ep in eps[:len(ends)]] == [b - a for a, b in zip(bounds[:-1], bounds[1:])]
        assert all(ep["complete"] for ep in eps[:len(ends)]) and (len(eps) == len(ends) or not eps[-1]["complete"])
        z = np.load(paths[k][:-4] + ".npz")
        assert int(z["episodes"]) == len(eps)
        for i, ep in enumerate(eps):
            for name in TrajectoryRecord.COLUMNS:
                assert tr.same_bits(z[f"{name}_{i}"], ep[name]), (name, i)
        cut = short.episodes(k)
        assert cut[-1]["truncated"] and sum(len(ep["reward"]) for ep in cut) == 3


def test_argument_errors_of_the_python_class():
    eng, _ = oracle_engine("QuadrupedPoseControl")
    for bad in ([3, 3], [0, N], [-1], [], list(range(257))):
        with pytest.raises(ValueError):
            TrajectoryRecord(eng, bad, 8)
    with pytest.raises(ValueError):
        TrajectoryRecord(eng, [0], 0)
    rec = TrajectoryRecord(eng, [5, 2], 8)
    assert tuple(rec.rows.shape) == (2, 8, 64) and rec.rows.dtype == torch.float32 and tuple(rec.header.shape) == (2, 4) and rec.header.dtype == torch.int32
    assert rec.ids.tolist() == [5, 2] and rec.episode_cap == 1
    covered = sorted(c for sl in TrajectoryRecord.COLUMNS.values() for c in range(sl.start, sl.stop))
    assert covered == list(range(64))


def test_header_constants_and_device_free_einval_cases():
    src = '#include <stdio.h>\n#include "lm_engine.h"\n#include "lm_policy.h"\nint main(){printf("%d %d %d\\n", LM_TRAJ_COLS, LM_TRAJ_MAX_ENVS, LM_ABI_VERSION);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c"); open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        cols, envs, abi = map(int, subprocess.check_output([exe]).split())
    assert cols == lmlib.TRAJ_COLS == tr.COLS == 64 and envs == lmlib.TRAJ_MAX_ENVS == 256 and abi == lmlib.ABI_VERSION == 5
    so = (lmlib.build_library(), lmlib.load_library())[1]
    for n in ("lm_rollout_set_trajectory_record", "lm_trajectory_update"):
        assert n in lmlib.EXPORTS and hasattr(so, n)
    assert so.lm_rollout_set_trajectory_record(None, None, 0, None, None, 0, 0) == -1 and b"lm_rollout_set_trajectory_record" in so.lm_last_error()
    assert so.lm_trajectory_update(None, None, 1, None, None, None, None, 1, 1, None) == -1 and b"lm_trajectory_update" in so.lm_last_error()
    hdr = open(os.path.join(ROOT, "include", "lm_policy.h")).read()
    assert re.search(r"SYNCHRONOUS", hdr) and re.search(r"TERMINAL state", hdr) and re.search(r"NOT world positions", hdr)
    # the state rows the device code restates are the ones of the step's header and of the Python mirror
    dyn = open(os.path.join(ROOT, "locomanipulationrl_amd", "csrc", "lm_dynamics.h")).read()
    dev = open(os.path.join(ROOT, "locomanipulationrl_amd", "csrc", "lm_traj_dev.h")).read()
    for name, row in (("Q", tr.Q), ("QD", tr.QD), ("LACT", tr.LACT), ("LTIP", tr.LTIP), ("GOAL", tr.GOAL)):
        assert int(re.search(rf"#define R_{name} (\d+)", dyn).group(1)) == row == int(re.search(rf"#define TRAJ_R_{name} (\d+)", dev).group(1))
    assert int(re.search(r"#define R_FB0 (\d+)", dyn).group(1)) == tr.FB0 and int(re.search(r"#define R_FB1 (\d+)", dyn).group(1)) == tr.FB1
