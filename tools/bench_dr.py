"""Cost of domain randomisation inside the step launch: k_step vs k_step_dr (YAML block of QuadrupedPoseControl.yaml) at 4096 envs, and what
the contact-material channel adds to k_step_dr (the same block + the feet's material_properties, redrawn every step in 64 buckets)."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import locomanipulationrl_amd as lm

res = {}
MATERIAL = {"articulation_views": {"robot_view": {"material_properties": {"on_interval": dict(
    frequency_interval=1, operation="scaling", distribution="uniform", distribution_parameters=[[1.0, 0.6, 1.0], [1.0, 1.4, 1.0]], num_buckets=64)}}}}
for name, ov in (("plain", None), ("randomised", {"task": {"domain_randomization": {"randomize": True}}}),
                 ("randomised_material", {"task": {"domain_randomization": {"randomize": True, "randomization_params": MATERIAL}}})):
    env = lm.make_env("QuadrupedPoseControl", num_envs=4096, overrides=ov)
    e = env._task.engine; N = 4096
    g = torch.Generator(device="cuda").manual_seed(0)
    pool = [torch.rand(N, 12, device="cuda", generator=g) * 2 - 1 for _ in range(16)]
    o = (torch.empty(N, 64, device="cuda"), torch.empty(N, 93, device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, dtype=torch.int64, device="cuda"), torch.empty(13, device="cuda"))
    for t in range(50): e.step(pool[t % 16], None, *o)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for t in range(500): e.step(pool[t % 16], None, *o)
    torch.cuda.synchronize(); res[name] = (time.perf_counter() - t0) / 500 * 1e6
    env.close()
print(json.dumps({"us_per_step": res, "overhead": res["randomised"] / res["plain"] - 1,
                  "material_overhead_on_k_step_dr": res["randomised_material"] / res["randomised"] - 1}))
