#!/usr/bin/env python3
"""Time the PPO update of the reference recipe (T 48, N 4096, num_obs 64, 5 epochs, 1 mini-batch) in both modes, on buffers of one real
fused rollout: the torch update() against the HIP update() (PPO(hip_update=True): lm_mlp_ppo_grad + lm_gae), and compute_gae against lm_gae.

    python tools/bench_ppo_update.py [--policy mlp|gnn] [--reps 20] [--warmup 3] [--out profiles/ppo_update_bench.json]

--policy gnn times the GraphPolicy's update the same way (PPO(gnn_hip_update=True): lm_gnn_ppo_grad + lm_gae, on QuadrupedPoseControlVertical) and
writes profiles/gnn_update_bench.json; the default, mlp, is unchanged.

Protocol: one process, two trainers on two engines with the same seed (identical rollouts), each warmed up; the two paths are timed
alternately (torch, hip, torch, hip, ...) with a device event on either side of each call, so clock and thermal drift hit both alike.  Every
repetition starts from the same trainer state (restored outside the timed region: an update changes the parameters, the scalers and the
learning rate).  Reported per path: median, quartiles, min, max, and the medians of the first and the second half of the repetitions, whose
difference is the run-to-run spread the comparison has to beat."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import locomanipulationrl_amd as lm
from locomanipulationrl_amd import distributed as D
from locomanipulationrl_amd.policies.mlp_model import SharedMLP, gae, ppo_grad_geometry
from locomanipulationrl_amd.train.ppo import PPO


def summary(ms):
    q = statistics.quantiles(ms, n=4)
    h = len(ms) // 2
    return {"median_ms": statistics.median(ms), "p25_ms": q[0], "p75_ms": q[2], "min_ms": min(ms), "max_ms": max(ms),
            "median_first_half_ms": statistics.median(ms[:h]), "median_second_half_ms": statistics.median(ms[h:]), "reps": len(ms)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=4096); ap.add_argument("--rollouts", type=int, default=48); ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20); ap.add_argument("--warmup", type=int, default=3); ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--policy", choices=("mlp", "gnn"), default="mlp")
    ap.add_argument("--out", default=None, help="default: profiles/ppo_update_bench.json (mlp), profiles/gnn_update_bench.json (gnn)")
    a = ap.parse_args()
    assert a.reps >= 2
    gnn = a.policy == "gnn"
    if a.out is None:
        a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gnn_update_bench.json" if gnn else "ppo_update_bench.json")
    tr = {}
    for mode in ("torch", "hip"):
        torch.manual_seed(a.seed)
        env = lm.make_env("QuadrupedPoseControlVertical" if gnn else "QuadrupedPoseControl", num_envs=a.num_envs, seed=a.seed)
        if gnn:
            from locomanipulationrl_amd.policies.graph_model import GraphPolicy
            ppo = PPO(env, GraphPolicy().to("cuda:0"), rollouts=a.rollouts, learning_epochs=a.epochs, gnn_hip_update=(mode == "hip"))
        else:
            ppo = PPO(env, SharedMLP(64).to("cuda:0"), rollouts=a.rollouts, learning_epochs=a.epochs, hip_update=(mode == "hip"))
        obs = env.reset()["obs"]
        obs, last_value, _ = ppo.collect(obs)                    # one real fused rollout fills the buffers both updates read
        tr[mode] = (env, ppo, last_value.clone(), ppo.state_dict())
    times = {"torch": [], "hip": []}
    for rep in range(a.warmup + a.reps):
        for mode in ("torch", "hip"):
            _, ppo, last_value, sd = tr[mode]
            ppo.load_state_dict(sd)
            ms = timed(lambda: ppo.update(last_value))
            if rep >= a.warmup:
                times[mode].append(ms)
    _, ppo, last_value, _ = tr["hip"]
    rew, val, dones = ppo.b_rew, ppo.b_val, ppo.rollout.dones
    dones_f = dones.float()
    gt = {"compute_gae": [], "lm_gae": []}
    for rep in range(a.warmup + a.reps):
        for name, fn in (("compute_gae", lambda: D.compute_gae(rew, val, dones_f, last_value, 0.99, 0.95)), ("lm_gae", lambda: gae(rew, val, dones, last_value, 0.99, 0.95))):
            ms = timed(fn)
            if rep >= a.warmup:
                gt[name].append(ms)
    B = a.rollouts * a.num_envs
    n_w = 256 * 64 + 128 * 256 + 64 * 128 + 13 * 64                 # weights: every one meets each sample in the forward, the delta and the dW product
    if gnn:
        from locomanipulationrl_amd.policies.graph_model import gnn_ppo_grad_geometry
        tile, groups = gnn_ppo_grad_geometry(B, "cuda:0")
        kern = {"mfma": "v_mfma_f32_16x16x4_f32", "tile": tile, "groups": groups}      # no FLOP count: the kernel recomputes activations, a count would flatter it
    else:
        tile, groups = ppo_grad_geometry(64, B, "cuda:0")
        kern = {"mfma": "v_mfma_f32_16x16x4_f32", "tile": tile, "groups": groups, "flop_per_call": 2 * 3 * n_w * B - 2 * 256 * 64 * B,
                "flop_note": "2 x (forward + delta + dW) x weights x samples, minus the delta product of layer 1 (no gradient flows into the observations)"}
    res = {"shape": {"T": a.rollouts, "N": a.num_envs, "B": B, "num_obs": 64, "epochs": a.epochs, "mini_batches": 1},
           "protocol": "one process, alternating torch / hip, device events around each call, state restored before each, warmup %d" % a.warmup,
           "update": {k: summary(v) for k, v in times.items()}, "gae": {k: summary(v) for k, v in gt.items()},
           "kernel": kern,
           "device": torch.cuda.get_device_name(0)}
    u = res["update"]
    spread = max(abs(u[m]["median_first_half_ms"] - u[m]["median_second_half_ms"]) for m in u)
    res["update_speedup_median"] = u["torch"]["median_ms"] / u["hip"]["median_ms"]
    res["update_run_to_run_spread_ms"] = spread
    res["hip_beats_torch_beyond_spread"] = bool(u["torch"]["median_ms"] - u["hip"]["median_ms"] > spread)
    if gnn:
        res["policy"] = "gnn"
        res["hip_p25_p75_entirely_below_torch"] = bool(u["hip"]["p75_ms"] < u["torch"]["p25_ms"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))
    for env, *_ in tr.values():
        env.close()


if __name__ == "__main__":
    main()
