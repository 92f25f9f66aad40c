"""Replay of recorded joint motions over a grid of held per-env physics parameters: every (recording, grid point) pair is one env of ONE
engine, driven along the recording by a lib.ReplayPlan and scored on the device (include/lm_policy.h, "replay of recorded joint motions").
What a parameter fit needs - the 0.8 x friction fit of DESIGN.md 2.1 ran one value per process on the CPU oracle - and, with joint logs of
a real robot in the recordings' format, a system-identification sweep over any of the 69 held rows.  On the PD-actuator tasks (custom controller, position control, position
drive) the recordings come with a command log - per recording the logged actions or the logged joint position targets - and the grid names
kp_scale, kd_scale and latency fit the actuator from it.

Layout: the locomotion recordings go on the block with the free base, the manipulation recordings on the block with the plate; inside a
block env = first + file x points + point, and each block is padded to a multiple of 16 with envs that take no part (-1).
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Sequence

import numpy as np

from ..lib import Engine, ReplayPlan, ReplayRecord
from .evaluate import sweep_env_params

KINDS = {"loco": 0, "mani": 1}          # kind of a recording -> mode of the block that replays it
WINDOW_ROWS = 17                        # the task's success streak (rows of PhysX's success window in the reference's recordings)


def replay_layout(names: Sequence[str], kinds: Dict[str, str], modes: Sequence[int], num_points: int, max_envs: Optional[int] = None) -> Dict:
    """Where every (recording, grid point) pair runs: {"num_envs", "split" (first env of the second block, None with one block), "env_rec" (N,)
    recording index or -1, "groups" (N,) grid point of the env (0 on padding), "env_of" {(name, point): env}}.  ValueError for a kind that is
    neither "loco" nor "mani", a recording whose kind no block of the engine has, an empty grid, or a layout beyond max_envs."""
    if num_points < 1:
        raise ValueError("the grid is empty: at least one point is needed")
    modes = [int(m) for m in modes]
    if len(modes) not in (1, 2) or len(set(modes)) != len(modes):
        raise ValueError(f"one block, or one locomotion and one manipulation block, are needed (modes {modes})")
    per_block: List[List[str]] = [[] for _ in modes]
    for n in names:
        k = kinds[n] if n in kinds else None
        if k not in KINDS:
            raise ValueError(f"recording {n!r}: its kind must be 'loco' or 'mani', not {k!r}")
        if KINDS[k] not in modes:
            raise ValueError(f"recording {n!r} is a {k} recording and the engine has no {k} block: it cannot be replayed on a block of the other kind")
        per_block[modes.index(KINDS[k])].append(n)
    sizes = [-(-(len(f) * num_points) // 16) * 16 for f in per_block]
    if len(modes) == 2:
        sizes = [max(s, 16) for s in sizes]          # a co-training engine needs both halves
    N = sum(sizes)
    if N < 1:
        raise ValueError("no recording to replay")
    if max_envs is not None and N > int(max_envs):
        raise ValueError(f"a grid of {num_points} points x {len(names)} recordings needs {N} envs and does not fit {int(max_envs)}")
    env_rec = np.full(N, -1, dtype=np.int32); groups = np.zeros(N, dtype=np.int64); env_of = {}
    index = {n: i for i, n in enumerate(names)}
    first = 0
    for files, size in zip(per_block, sizes):
        for f, n in enumerate(files):
            for p in range(num_points):
                e = first + f * num_points + p
                env_rec[e] = index[n]; groups[e] = p; env_of[(n, p)] = e
        first += size
    return dict(num_envs=N, split=sizes[0] if len(modes) == 2 else None, env_rec=env_rec, groups=groups, env_of=env_of)


def as_replay_run(s: Dict, T: int, window_rows: int = WINDOW_ROWS) -> Dict:
    """One env's summary in the shape of the host replay's result (the keys its checks read): None for a termination or success that never
    came, `rd` holding the first row's rot_dist and `rd_rec` the smallest over the recorded rows."""
    return dict(T=int(T), succ_row=int(T) - window_rows, rows=int(s["rows"]), row0_err=float(s["row0_err"]), qerr=float(s["qerr"]), rms=float(s["rms"]),
                mean_abs=float(s["mean_abs"]), tracked=float(s["tracked"]), early=float(s["early"]), done_at=int(s["done_at"]) if s["done_at"] >= 0 else None,
                goal=int(s["goal"]), first_succ=int(s["first_succ"]) if s["first_succ"] >= 0 else None, in_window=int(s["in_window"]),
                rd=np.array([float(s["rd_first"])]), rd_rec=np.array([float(s["min_rd"])]), ret=float(s["return"]), window_return=float(s["window_return"]))


def leave_one_out(table: Dict, names: Sequence[str]) -> List:
    """[(held-out file, grid point with the most shared window rows on the other files - the first of the table on ties -, held-out rows
    there)] for a table {point: [rows per file, in the order of `names`]}."""
    out = []
    keys = list(table)
    for k, name in enumerate(names):
        score = {p: sum(v for j, v in enumerate(table[p]) if j != k) for p in keys}
        best = max(keys, key=lambda p: score[p])
        out.append((name, best, table[best][k]))
    return out


def sweep_engine(robot_model, params, layout: Dict, points: Sequence[Dict[str, float]], seed: int = 0, engine_cls=Engine):
    """A fresh engine of the layout's size with the grid held: the blocks with dr_enabled and every channel off (the randomised kernels are the
    ones that apply held rows), env params enabled, env e held at points[layout["groups"][e]] through sweep_env_params."""
    off = lambda chans: [dataclasses.replace(c, enabled=0) for c in chans]
    params = [dataclasses.replace(p, dr_enabled=1, dr=off(p.dr), dr_mat=off(p.dr_mat), dr_reset=off(p.dr_reset), dr_mass=off(p.dr_mass), dr_actuator=off(p.dr_actuator))
              for p in params]
    N, split = layout["num_envs"], layout["split"]
    eng = engine_cls(robot_model, params, N, split_env=split, seed=seed)
    try:
        eng.enable_env_params()
        block = lambda e: params[1 if (split and e >= split) else 0]
        held = sweep_env_params(points, layout["groups"], body_masses=np.asarray([robot_model.mass[i] for i in robot_model.table_body_order()], dtype=np.float64),
                                kp=np.asarray([block(e).pd_kp for e in range(N)], dtype=np.float64), kd=np.asarray([block(e).kd for e in range(N)], dtype=np.float64))
        if held:
            eng.set_env_params(**held)
    except Exception:
        eng.close()
        raise
    return eng


def replay_sweep(robot_model, params, recordings: Dict[str, np.ndarray], kinds: Dict[str, str], points: Sequence[Dict[str, float]], servo: bool = False,
                 hold: int = 2, window_rows: int = WINDOW_ROWS, succ_thresh: float = 0.15, track_tol: float = 1e-3, score_files: Optional[Sequence[str]] = None,
                 seed: int = 0, max_envs: Optional[int] = None, engine_cls=Engine, actions: Optional[Dict[str, np.ndarray]] = None,
                 targets: Optional[Dict[str, np.ndarray]] = None) -> Dict:
    """Replay every recording at every grid point on one fresh engine and score it on the device.  `params`: the engine's parameter block(s)
    (one, or a locomotion and a manipulation block); `recordings` {name: (L, 12)}; `kinds` {name: "loco" | "mani"}; `points` a list of
    {sweep name: value} (train.evaluate.sweep_grid; the names of SWEEP_NAMES).  The engine is created with dr_enabled and no channel, env
    params are enabled and the grid is held through sweep_env_params - the held `mu` row is mu_env itself, so mu = 0.8 is the shipped
    point.  Returns {"points", "runs": {point index: {file: summary in the shape of as_replay_run}}, "in_window": {point index: [rows inside
    the recorded success window per file of `score_files`]}, "shared": {point index: their sum}, "leave_one_out": the picks over `score_files`,
    "files", "score_files", "layout", "steps"}.  `score_files` defaults to every recording.
    PD-actuator blocks (lib.ReplayPlan) take the command log of every recording: `actions` {name: (L, 12)} (the logged actions; a trajectory
    record's last_actions) or `targets` {name: (L, 12)} (the logged joint position targets), or servo=True (the recordings are the targets);
    every summary then also carries `saturated` and `cmd_err`."""
    names = list(recordings)
    for what, table in (("actions", actions), ("targets", targets)):
        if table is not None and sorted(table) != sorted(names):
            raise ValueError(f"{what}: one (L, 12) array per recording is needed, under the recordings' names (missing {sorted(set(names) - set(table))}, "
                             f"unknown {sorted(set(table) - set(names))})")
    points = [dict(p) for p in points]
    lay = replay_layout(names, kinds, [p.mode for p in params], len(points), max_envs)
    score_files = list(names if score_files is None else score_files)
    missing = [n for n in score_files if n not in recordings]
    if missing:
        raise ValueError(f"score_files names recordings that are not there: {missing}")
    eng = sweep_engine(robot_model, params, lay, points, seed=seed, engine_cls=engine_cls)
    try:
        plan = ReplayPlan(eng, [recordings[n] for n in names], lay["env_rec"], servo=servo, hold=hold, window_rows=window_rows, succ_thresh=succ_thresh,
                          track_tol=track_tol, actions=None if actions is None else [actions[n] for n in names],
                          targets=None if targets is None else [targets[n] for n in names])
        record = plan.run(ReplayRecord(eng))
        summ = record.summary()
        steps = plan.steps
        plan.close()
    finally:
        eng.close()
    def one(n, p):
        e = lay["env_of"][(n, p)]
        return dict(as_replay_run({k: v[e] for k, v in summ.items()}, len(recordings[n]), window_rows), saturated=int(summ["saturated"][e]), cmd_err=float(summ["cmd_err"][e]))
    runs = {p: {n: one(n, p) for n in names} for p in range(len(points))}
    table = {p: [runs[p][n]["in_window"] for n in score_files] for p in range(len(points))}
    return dict(points=points, runs=runs, in_window=table, shared={p: int(sum(v)) for p, v in table.items()}, leave_one_out=leave_one_out(table, score_files),
                files=names, score_files=score_files, layout=lay, steps=steps)
