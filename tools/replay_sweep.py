#!/usr/bin/env python3
"""Replay recorded joint trajectories over a grid of held per-env physics parameters on ONE engine and score every (recording, grid point)
pair on the device (train/replay.py, include/lm_policy.h "replay of recorded joint motions"): a parameter fit, or system identification
from joint logs, in one run.
    python tools/replay_sweep.py --recordings tests/golden/npy_traj.npz [--npy FILE:loco|mani ...] --sweep mu=0.5:1.2:8 [--sweep ...] [--servo] [--out JSON]
    python tools/replay_sweep.py --task QuadrupedPoseControlCustomController --log robot_log.npz --sweep kp_scale=0.5:2:16 --sweep latency=0:4:5
--recordings takes an .npz of (L, 12) arrays (the reference's RECORD_JOINT files: byte-identical duplicates are replayed once; an array is a
manipulation recording when the part of its name in front of "from" contains "mani"), --npy single files as TrajectoryRecord.save_npy and the
reference write them.  --sweep NAME=LO:HI:K as tools/eval_policy.py (several form their Cartesian product; mu is the contact coefficient
itself: 0.8 is the shipped value).  The blocks are those of --task (any shipped task YAML; default: the co-training task the reference recorded,
JointLocomanipulation) with the goal fixed at --goal (default on the default task: the goal the committed reference code recorded under; "task",
the default on any other task, keeps the task's range).  --log takes an .npz of a command-and-joint log for the PD-actuator tasks (custom
controller, position control): per recording NAME the keys q_NAME (L, 12) - the measured joints - and ONE of actions_NAME (L, 12) - the action
of every control step, row 0 the reset step's - or targets_NAME (L, 12) - the joint position targets commanded for every step, in the joints'
order; every recording of a file carries the same of the two.  --score names the
recordings the window table and the leave-one-out picks are taken over; --repeat runs the sweep several times in one process (timing).
Prints one JSON line: per grid point its values, the rows inside the recorded success window per file and their sum, per file the replay's
summary; the leave-one-out picks; the wall time of the sweep (engine creation to summary) in seconds."""
import argparse, dataclasses, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


TASK = "JointLocomanipulation"


def kind_of(name):
    return "mani" if "mani" in name.split("from")[0] else "loco"


def load_recordings(npz, npy):
    recs, kinds = {}, {}
    if npz:
        g = np.load(npz)
        for k in g.files:
            a = g[k].astype(np.float64)
            if any(a.shape == b.shape and np.array_equal(a, b) for b in recs.values()):
                continue
            recs[k] = a; kinds[k] = kind_of(k)
    for spec in npy:
        path, _, kind = spec.rpartition(":")
        if not path or kind not in ("loco", "mani"):
            raise SystemExit(f"--npy {spec!r}: FILE:loco or FILE:mani is needed")
        name = os.path.splitext(os.path.basename(path))[0]
        recs[name] = np.load(path).astype(np.float64); kinds[name] = kind
    return recs, kinds


def load_log(path, recs, kinds):
    """The recordings of a command-and-joint log added to recs / kinds; returns ("actions" | "targets", {name: (L, 12)})."""
    g = np.load(path)
    names = [k[2:] for k in g.files if k.startswith("q_")]
    if not names:
        raise SystemExit(f"--log {path}: no q_NAME array")
    which = [w for w in ("actions", "targets") if all(f"{w}_{n}" in g.files for n in names)]
    if len(which) != 1:
        raise SystemExit(f"--log {path}: every recording needs actions_NAME, or every recording targets_NAME (and not both)")
    for n in names:
        recs[n] = g["q_" + n].astype(np.float64); kinds[n] = kind_of(n)
    return which[0], {n: g[f"{which[0]}_{n}"].astype(np.float64) for n in names}


def jsonable(r):
    return {k: (v.tolist() if isinstance(v, np.ndarray) else None if isinstance(v, float) and v != v else v) for k, v in r.items()}          # (a PD plan has no `early`: nan)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", default=None, help=".npz of (L, 12) joint trajectories")
    ap.add_argument("--npy", action="append", default=[], metavar="FILE:loco|mani", help="one (L, 12) .npy and the block that replays it (repeatable)")
    ap.add_argument("--sweep", action="append", default=[], metavar="NAME=LO:HI:K", help="hold a grid of per-env parameters (repeatable: Cartesian product)")
    ap.add_argument("--task", default=TASK, help="the task YAML whose parameter blocks replay the recordings")
    ap.add_argument("--log", default=None, help=".npz command-and-joint log of a PD-actuator task: q_NAME and actions_NAME or targets_NAME per recording")
    ap.add_argument("--goal", default=None, help="roll,pitch,yaw the recordings were made under, or 'task' (default: 0.2,0.2,0.785 on the default task, 'task' otherwise)")
    ap.add_argument("--servo", action="store_true", help="steer the joints back onto the recording every step instead of replaying the recovered actions")
    ap.add_argument("--repeat", type=int, default=1, help="run the sweep this many times (wall times are listed)")
    ap.add_argument("--score", default=None, help="comma-separated recordings the window table and the leave-one-out picks are taken over (default: all)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    from locomanipulationrl_amd.lib import build_library
    from locomanipulationrl_amd.model.robot_model import load_model
    from locomanipulationrl_amd.train.evaluate import parse_sweep, sweep_grid
    from locomanipulationrl_amd.train.replay import replay_sweep
    from locomanipulationrl_amd.utils.config import SimConfig, load_config
    from locomanipulationrl_amd.utils.task_util import task_map
    try:
        points = sweep_grid([parse_sweep(x) for x in a.sweep]) if a.sweep else [{}]
    except ValueError as e:
        raise SystemExit(str(e))
    recs, kinds = load_recordings(a.recordings, a.npy)
    command = {}
    if a.log:
        if recs:
            raise SystemExit("--log carries its own recordings: it does not combine with --recordings / --npy")
        which, table = load_log(a.log, recs, kinds)
        command = {which: table}
    if not recs:
        raise SystemExit("no recording: give --recordings, --npy or --log")
    if a.task not in task_map():
        raise SystemExit(f"--task {a.task!r}: one of {sorted(task_map())}")
    task = task_map()[a.task](name=a.task, sim_config=SimConfig(load_config(a.task, num_envs=32)), env=None)
    params = task.engine_params()
    goal_arg = a.goal if a.goal is not None else ("0.2,0.2,0.785" if a.task == TASK else "task")
    if goal_arg != "task":
        goal = [float(x) for x in goal_arg.split(",")]
        params = [dataclasses.replace(p, goal_lo=goal, goal_hi=goal) for p in params]
    build_library()
    rm = load_model(task.model_asset)
    score = a.score.split(",") if a.score else None
    walls = []
    try:
        for _ in range(max(a.repeat, 1)):
            t0 = time.perf_counter()
            out = replay_sweep(rm, params, recs, kinds, points, servo=a.servo, score_files=score, **command)
            walls.append(time.perf_counter() - t0)
    except ValueError as e:
        raise SystemExit(str(e))
    line = json.dumps({"task": a.task, "servo": bool(a.servo), "num_envs": out["layout"]["num_envs"], "steps": out["steps"], "files": out["files"],
                       "score_files": out["score_files"],
                       "points": [{"point": out["points"][p], "in_window": out["in_window"][p], "shared": out["shared"][p],
                                   "runs": {n: jsonable(r) for n, r in out["runs"][p].items()}} for p in range(len(out["points"]))],
                       "leave_one_out": [{"held_out": n, "point": out["points"][p], "rows": rows} for n, p, rows in out["leave_one_out"]],
                       "wall_s": walls[-1], "walls_s": walls})
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
