#!/usr/bin/env python3
"""Replay recorded joint trajectories over a grid of held per-env physics parameters on ONE engine and score every (recording, grid point)
pair on the device (train/replay.py, include/lm_policy.h "replay of recorded joint motions"): a parameter fit, or system identification
from joint logs, in one run.
    python tools/replay_sweep.py --recordings tests/golden/npy_traj.npz [--npy FILE:loco|mani ...] --sweep mu=0.5:1.2:8 [--sweep ...] [--servo] [--out JSON]
--recordings takes an .npz of (L, 12) arrays (the reference's RECORD_JOINT files: byte-identical duplicates are replayed once; an array is a
manipulation recording when the part of its name in front of "from" contains "mani"), --npy single files as TrajectoryRecord.save_npy and the
reference write them.  --sweep NAME=LO:HI:K as tools/eval_policy.py (several form their Cartesian product; mu is the contact coefficient
itself: 0.8 is the shipped value).  The blocks are those of the co-training task the reference recorded (JointLocomanipulation) with the goal
fixed at --goal (default: the goal the committed reference code recorded under; "task" keeps the task's range).  --score names the
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
    if not recs:
        raise SystemExit("no recording: give --recordings and / or --npy")
    return recs, kinds


def jsonable(r):
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in r.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", default=None, help=".npz of (L, 12) joint trajectories")
    ap.add_argument("--npy", action="append", default=[], metavar="FILE:loco|mani", help="one (L, 12) .npy and the block that replays it (repeatable)")
    ap.add_argument("--sweep", action="append", default=[], metavar="NAME=LO:HI:K", help="hold a grid of per-env parameters (repeatable: Cartesian product)")
    ap.add_argument("--goal", default="0.2,0.2,0.785", help="roll,pitch,yaw the recordings were made under, or 'task'")
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
    task = task_map()[TASK](name=TASK, sim_config=SimConfig(load_config(TASK, num_envs=32)), env=None)
    params = task.engine_params()
    if a.goal != "task":
        goal = [float(x) for x in a.goal.split(",")]
        params = [dataclasses.replace(p, goal_lo=goal, goal_hi=goal) for p in params]
    build_library()
    rm = load_model(task.model_asset)
    score = a.score.split(",") if a.score else None
    walls = []
    try:
        for _ in range(max(a.repeat, 1)):
            t0 = time.perf_counter()
            out = replay_sweep(rm, params, recs, kinds, points, servo=a.servo, score_files=score)
            walls.append(time.perf_counter() - t0)
    except ValueError as e:
        raise SystemExit(str(e))
    line = json.dumps({"task": TASK, "servo": bool(a.servo), "num_envs": out["layout"]["num_envs"], "steps": out["steps"], "files": out["files"],
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
