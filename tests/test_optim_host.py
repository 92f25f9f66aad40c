"""The device optimiser step's host side, without a GPU: the float64 reference equals torch's own clip + Adam in float64 and the rule of
update(), the new symbols are exported with the ABI stamp unchanged and refuse bad arguments before anything is launched, and
hip_optimizer refuses to run without a fused update."""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys
import tempfile

import pytest
import torch

import locomanipulationrl_amd as lm
import optim_reference as R
from conftest import GOLDEN, ROOT
from locomanipulationrl_amd import lib as lmlib
from locomanipulationrl_amd.policies.mlp_model import SharedMLP
from locomanipulationrl_amd.train.ppo import PPO
from oracle_backend import oracle_engine_factory


@pytest.fixture(scope="module")
def so():
    lmlib.build_library()
    return lmlib.load_library()


# ------------------------------------------------------------------------------------------------ the reference against torch
@pytest.mark.parametrize("n", (1, 65, 10190))
@pytest.mark.parametrize("scale", ("below", "above", "zero"))
def test_reference_equals_torch_float64_over_three_steps(n, scale):
    c = R.make_case(n, scale)
    h = R.HYPER
    want = R.torch_steps(c.p, c.grads, c.m, c.v, torch.float64, **h)
    p, m, v, step = c.p, c.m, c.v, 0
    norm0 = float(c.grads[0].double().norm())
    assert (norm0 < h["max_norm"]) if scale == "below" else ((norm0 > h["max_norm"]) if scale == "above" else norm0 == 0.0)
    for k, g in enumerate(c.grads):
        p, m, v, step, norm, coef = R.clip_adam_step64(p, g, m, v, step, h["lr"], h["beta1"], h["beta2"], h["eps"], h["max_norm"])
        assert step == k + 1 and norm == pytest.approx(float(g.double().norm()), rel=1e-14)
        assert coef == (1.0 if scale != "above" else pytest.approx(h["max_norm"] / (norm + 1e-6), rel=1e-15))
        for name, got, ref in (("p", p, want[k][0]), ("exp_avg", m, want[k][1]), ("exp_avg_sq", v, want[k][2])):
            assert R.rel(got, ref) <= 1e-12, (n, scale, k, name, R.rel(got, ref))
    if scale == "zero":
        assert torch.equal(p, c.p.double()) and not bool(m.any()) and not bool(v.any())


def test_reference_clamp_floors_its_range_only():
    c = R.make_case(65, "below")
    h = R.HYPER
    free = R.clip_adam_step64(c.p, c.grads[0], c.m, c.v, 0, h["lr"], h["beta1"], h["beta2"], h["eps"], h["max_norm"])[0]
    got = R.clip_adam_step64(c.p, c.grads[0], c.m, c.v, 0, h["lr"], h["beta1"], h["beta2"], h["eps"], h["max_norm"], clamp=(60, 5, 0.0))[0]
    assert torch.equal(got[:60], free[:60]) and torch.equal(got[60:], free[60:].clamp_min(0.0)) and bool((free[60:] < 0).any()) and bool((free[60:] > 0).any())


# ------------------------------------------------------------------------------------------------ the reference against the epoch loop
def rule_of_update(lr, kl, kl_thr, max_lr):
    """The lines of PPO.update, transcribed (self.lr -> lr, self.kl_thr -> kl_thr, self.max_lr -> max_lr)."""
    if kl_thr > 0:
        if kl > kl_thr * 2: lr = max(lr / 1.5, 1e-6)
        elif kl < kl_thr / 2: lr = min(lr * 1.5, max_lr)
    return lr


def test_kl_rule_equals_the_rule_of_update():
    seen = set()
    for name, lr, kls, thr, lr_min, lr_max, expect in R.kl_table():
        assert lr_min == 1e-6
        want = lr
        for i, kl in enumerate(kls):
            new = R.kl_rule(lr, [kl], thr, lr_min, lr_max); want = rule_of_update(want, kl, thr, lr_max)
            assert new == want, (name, i, new, want)
            if expect is not None:
                assert (new > lr) - (new < lr) == expect[i], (name, kl, lr, new)
            lr = new
        seen.add(lr)
    assert 1e-6 in seen and 1e-2 in seen, seen      # the two walks arrive at the floor and at the cap
    # a mean of three is the double mean of the values
    vals = R.spread3(2 * R.THR * 1.001)
    assert R.kl_rule(3e-4, vals, R.THR, 1e-6, 1e-2) == rule_of_update(3e-4, (vals[0] + vals[1] + vals[2]) / 3, R.THR, 1e-2) == 3e-4 / 1.5


# ------------------------------------------------------------------------------------------------ ABI and validation
NEW = ("lm_optim_state_len", "lm_optim_state_init", "lm_adam_clip_step", "lm_kl_adaptive_lr")


def test_new_symbols_are_exported_and_the_abi_stamp_is_unchanged(so):
    for n in NEW:
        assert n in lmlib.EXPORTS and hasattr(so, n), n
    assert so.lm_abi_version() == 5 == lmlib.ABI_VERSION
    want = json.load(open(os.path.join(GOLDEN, "ppo_update_parent_cpu.json")))
    assert C.sizeof(lmlib.LmParams) == want["sizeof_lm_params"]
    assert so.lm_optim_state_len() == 8


def test_hyper_struct_layout_matches_c():
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "lm_policy.h"\nint main(){printf("%zu %zu %zu %zu %d\\n", sizeof(lm_optim_hyper), ' \
          'offsetof(lm_optim_hyper, max_norm), offsetof(lm_optim_hyper, clamp_offset), offsetof(lm_optim_hyper, clamp_min), LM_OPTIM_STATE);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c"); open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        size, o_norm, o_off, o_min, n_state = map(int, subprocess.check_output([exe]).split())
    H = lmlib.LmOptimHyper
    assert (C.sizeof(H), H.max_norm.offset, H.clamp_offset.offset, H.clamp_min.offset) == (size, o_norm, o_off, o_min) and n_state == 8


def test_entry_points_refuse_bad_arguments_without_a_device(so):
    """Host arrays stand in for device blocks: every call below is refused before a launch (and before a pointer is followed)."""
    f = lambda: (C.c_float * 72)()
    p, g, m, v, kl = f(), f(), f(), f(), f()
    state = (C.c_double * 8)()
    hp = lambda off=0, cnt=0: lmlib.LmOptimHyper(0.9, 0.999, 1e-8, 1.0, off, cnt, 0.0, 0)
    ref = C.byref
    assert so.lm_optim_state_init(None, 3e-4, 0.0, None) == -1 and b"lm_optim_state_init" in so.lm_last_error()
    assert so.lm_optim_state_init(state, 3e-4, -1.0, None) == -1
    good = [p, g, m, v, 65, state, ref(hp()), None]
    for i in (0, 1, 2, 3, 5, 6):
        a = list(good); a[i] = None
        assert so.lm_adam_clip_step(*a) == -1 and b"null" in so.lm_last_error(), i
    for n in (0, -5):
        a = list(good); a[4] = n
        assert so.lm_adam_clip_step(*a) == -1 and b"n must be" in so.lm_last_error(), n
    for off, cnt in ((60, 6), (65, 1), (-1, 2), (0, 66), (0, -1), (2 ** 31 - 1, 2 ** 31 - 1)):
        a = list(good); a[6] = ref(hp(off, cnt))
        assert so.lm_adam_clip_step(*a) == -1 and b"clamp" in so.lm_last_error(), (off, cnt)
    a = list(good); a[6] = ref(hp(60, 5))
    assert so.lm_adam_clip_step(*a) == -1 and b"clamp" not in so.lm_last_error()       # a good range: refused further on, as host memory
    assert so.lm_kl_adaptive_lr(None, kl, 1, 0.012, 1e-6, 1e-2, None) == -1 and so.lm_kl_adaptive_lr(state, None, 1, 0.012, 1e-6, 1e-2, None) == -1
    assert so.lm_kl_adaptive_lr(state, kl, 0, 0.012, 1e-6, 1e-2, None) == -1 and b"count" in so.lm_last_error()
    assert so.lm_kl_adaptive_lr(state, kl, 1, 0.012, 1e-6, 1e-2, None) == -1            # host memory
    assert list(state) == [0.0] * 8 and not any(p) and not any(m)


# ------------------------------------------------------------------------------------------------ refusals
def test_hip_optimizer_needs_a_fused_update_and_a_device():
    env = lm.make_env("QuadrupedPoseControl", num_envs=16, engine_factory=oracle_engine_factory, sim_device="cpu", rl_device="cpu")
    with pytest.raises(ValueError, match="hip_update=True"):
        PPO(env, SharedMLP(), rollouts=6, hip_inference=False, hip_optimizer=True)
    with pytest.raises(ValueError, match="HIP device"):
        PPO(env, SharedMLP(), rollouts=6, hip_inference=False, hip_update=True, hip_optimizer=True)
    ppo = PPO(env, SharedMLP(), rollouts=6, hip_inference=False)
    assert not ppo.hip_optimizer


def test_wrappers_have_no_cpu_fallback():
    from locomanipulationrl_amd.policies import optim
    with pytest.raises(RuntimeError, match="HIP device"):
        optim.optim_state("cpu", 3e-4)
    z = torch.zeros(8)
    with pytest.raises(RuntimeError, match="HIP device"):
        optim.adam_clip_step(z, z, z, z, torch.zeros(8, dtype=torch.float64))


def test_train_tool_refuses_hip_optimizer_without_hip_update(monkeypatch, capsys):
    spec = importlib.util.spec_from_file_location("train_ppo_tool", os.path.join(ROOT, "tools", "train_ppo.py"))
    tool = importlib.util.module_from_spec(spec); spec.loader.exec_module(tool)
    monkeypatch.setattr(sys, "argv", ["train_ppo.py", "--hip-optimizer", "--timesteps", "48"])
    with pytest.raises(SystemExit) as e:
        tool.main()
    assert e.value.code != 0 and "--hip-update" in capsys.readouterr().err
