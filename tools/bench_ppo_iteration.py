#!/usr/bin/env python3
"""Time one whole PPO iteration (collect() + update()) of the reference recipe (T 48, N 4096, num_obs 64, 5 epochs, 1 mini-batch) on two paths:
  A  hip_update + hip_optimizer                      every iteration packs the parameters with torch (blocking range checks), prepares the batch
                                                     with torch and copies the statistics to the host
  B  A + hip_prepare, update(last_value, fetch=False)  the pack, the scalers and the batch normalisation are launches of csrc/lm_prepare.hip and
                                                     nothing waits for the host

    python tools/bench_ppo_iteration.py [--policy mlp|gnn] [--block 10] [--reps 20] [--warmup 3] [--out profiles/ppo_iteration_bench.json]

The timed unit is the WALL CLOCK of a block of K iterations with one torch.cuda.synchronize() after the block, divided by K: what the change
removes is host-side (blocking reads, small launches), and device events would not see a host that runs behind an idle device.  The preparation
phase of update() (all-gather, advantage normalisation, both scalers, the normalisation of the batch) is also recorded by device events through
PPO.phase_marks, in blocks of their own after the wall-clock blocks (recording events adds host work to the iteration).

Protocol (that of tools/bench_ppo_update.py): one process, two trainers of one seed on two engines, each warmed up; the two paths are timed
alternately (A, B, A, B, ...), so clock and thermal drift hit both alike.  Training goes on across the blocks: both trainers walk the same
number of iterations from the same seed.  Reported per path: median, quartiles, min, max, and the medians of the first and the second half of
the blocks, whose difference is the run-to-run spread the comparison has to beat."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import locomanipulationrl_amd as lm
from locomanipulationrl_amd.policies.mlp_model import SharedMLP
from locomanipulationrl_amd.train.ppo import PPO


def summary(ms):
    q = statistics.quantiles(ms, n=4)
    h = len(ms) // 2
    return {"median_ms": statistics.median(ms), "p25_ms": q[0], "p75_ms": q[2], "min_ms": min(ms), "max_ms": max(ms),
            "median_first_half_ms": statistics.median(ms[:h]), "median_second_half_ms": statistics.median(ms[h:]), "reps": len(ms)}


class Path:
    def __init__(self, a, prepare):
        gnn = a.policy == "gnn"
        torch.manual_seed(a.seed)
        self.env = lm.make_env("QuadrupedPoseControlVertical" if gnn else "QuadrupedPoseControl", num_envs=a.num_envs, seed=a.seed)
        if gnn:
            from locomanipulationrl_amd.policies.graph_model import GraphPolicy
            model, kw = GraphPolicy().to("cuda:0"), {"gnn_hip_update": True}
        else:
            model, kw = SharedMLP(64).to("cuda:0"), {"hip_update": True}
        self.ppo = PPO(self.env, model, rollouts=a.rollouts, learning_epochs=a.epochs, hip_optimizer=True, hip_prepare=prepare, **kw)
        self.fetch = not prepare
        self.obs = self.env.reset()["obs"]

    def iterate(self, k):
        ppo = self.ppo
        for _ in range(k):
            self.obs, last_value, _ = ppo.collect(self.obs)
            ppo.update(last_value) if self.fetch else ppo.update(last_value, fetch=False)

    def wall_block(self, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.iterate(k)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / k

    def phase_block(self, k):
        """Device-event times (ms) of update()'s phases over k iterations: {phase: [k values]}"""
        out = {"gae": [], "normalise": [], "epochs": []}
        for _ in range(k):
            self.ppo.phase_marks = []
            self.iterate(1)
            marks, self.ppo.phase_marks = self.ppo.phase_marks, None
            torch.cuda.synchronize()
            for (_, e0), (name, e1) in zip(marks, marks[1:]):
                out[name].append(e0.elapsed_time(e1))
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=4096); ap.add_argument("--rollouts", type=int, default=48); ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--block", type=int, default=10, help="K: iterations per timed block"); ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3); ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--policy", choices=("mlp", "gnn"), default="mlp")
    ap.add_argument("--out", default=None, help="default: profiles/ppo_iteration_bench.json (mlp), profiles/gnn_iteration_bench.json (gnn)")
    a = ap.parse_args()
    assert a.reps >= 2 and a.block >= 1
    if a.out is None:
        a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", ("gnn" if a.policy == "gnn" else "ppo") + "_iteration_bench.json")
    paths = {"A_hip_optimizer": Path(a, False), "B_hip_prepare": Path(a, True)}
    wall = {m: [] for m in paths}
    for rep in range(a.warmup + a.reps):
        for m, p in paths.items():
            ms = p.wall_block(a.block)
            if rep >= a.warmup:
                wall[m].append(ms)
    phases = {m: {"gae": [], "normalise": [], "epochs": []} for m in paths}
    for rep in range(2):
        for m, p in paths.items():
            for k, v in p.phase_block(a.block).items():
                phases[m][k] += v
    p_b = paths["B_hip_prepare"].ppo
    p_b.state_dict()      # the deferred range check of path B: raises if the pack kernel flagged a weight
    res = {"policy": a.policy, "shape": {"T": a.rollouts, "N": a.num_envs, "B": a.rollouts * a.num_envs, "num_obs": 64, "epochs": a.epochs, "mini_batches": 1},
           "protocol": "one process, alternating A / B, wall clock of a block of %d iterations (collect + update) with one synchronize after the block, "
                       "per-iteration time = block time / %d, warmup %d blocks; training continues across blocks" % (a.block, a.block, a.warmup),
           "iteration": {m: summary(v) for m, v in wall.items()},
           "phases": {m: {k: summary(v) for k, v in ph.items()} for m, ph in phases.items()},
           "phases_note": "device events at update()'s phase boundaries in blocks of their own after the wall-clock blocks: gae | all-gather, advantage "
                          "normalisation, scalers, batch normalisation (B: lm_ppo_batch_stats + lm_ppo_batch_apply) | epoch loop",
           "iterations_per_path": (a.warmup + a.reps + 2) * a.block,
           "device": torch.cuda.get_device_name(0)}
    A, B = res["iteration"]["A_hip_optimizer"], res["iteration"]["B_hip_prepare"]
    res["B_minus_A_median_ms"] = B["median_ms"] - A["median_ms"]
    res["B_drift_ms"] = abs(B["median_first_half_ms"] - B["median_second_half_ms"])
    res["quartile_ranges_disjoint"] = bool(B["p75_ms"] < A["p25_ms"] or A["p75_ms"] < B["p25_ms"])
    # the rule of DESIGN.md 5.4: an improvement only if the quartile ranges are disjoint and the gap exceeds B's own first-half / second-half difference
    res["hip_prepare_is_an_improvement"] = bool(B["p75_ms"] < A["p25_ms"] and A["median_ms"] - B["median_ms"] > res["B_drift_ms"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))
    for p in paths.values():
        p.env.close()


if __name__ == "__main__":
    main()
