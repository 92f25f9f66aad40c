"""The task layer of the kernels - task_eval<MODE, VAR> with the action clamp and the swing/extension integration in front of it and the shared tail
write_outputs behind it (csrc/lm_task.h) - against the float64 oracle at its branch points (states of tests/task_states.py):
the success threshold, the counter machine, the quaternion sign flips and the antipodal goal, every joint band of every limb, every fall cause
of every limb, the ordering of the fall penalty, the timeout, the three clamps, the rotation-decrease carry and the success-rate windows at a
roll - with every env of a wavefront on the branch, every second one, and exactly one per wavefront at another lane position (and another limb) each.
test_task_states_host.py proves on the CPU that the states take those branches, that the float32 oracle takes the same ones (zero disagreements),
and that the float64 oracle reproduces the reference's own Python on them (tests/golden/task_branches.npz); what is left to miss here is the kernel.

  a. lm_task_eval (k_task_eval) on every scenario x layout: all integer outputs equal on every env, last_actions equal bit for bit, float outputs
     per group within K_TASK x gap;
  b. lm_task_eval against the fixture directly, to the tolerances of test_task_layer_against_reference_golden;
  c. the step kernels' own instances of the template: lm_post_physics (k_step, k_step_pd) on physical states whose kinematics put a knee, a corner
     or the base PHYS_MARGIN to either side of its threshold, and lm_step on every kernel family the host can select (the engine is asked which
     one it runs) against Oracle.step on the scenarios one step of physics cannot move: timeout, consecutive-success reset, window roll, action
     clamp.

Tolerance of the float comparison, per group (obs, states, reward, the eleven terms, extras, task rows): K_TASK x gap, where gap is the largest
|f32 oracle - f64 oracle| of the group on the same states, floored at 8 float32 epsilons of the group's largest magnitude.  K_TASK is the next
power of two above the largest ratio max |gpu - f64| / gap measured on the MI355X, at most 32; the tests print every ratio, and a ratio above 32
is a finding, not a bound to widen.  Measured: see K_TASK below.
The published success rates are compared to one float32 step: the engine is built without correctly rounded float32 division, the reference
divides in float64."""
import os

import numpy as np
import pytest
import torch

import task_states as ts
from conftest import GOLDEN
from oracle_backend import OracleEngine

pytestmark = pytest.mark.gpu

# Largest ratios measured on the MI355X, one run over all 461 cases of a. (every scenario x layout at N = 64, eleven at N = 50; 3161 group ratios with
# those of c.): obs 0.14 (rot_decrease_below_then_above_loco_cc all, second evaluation), states 1.00, reward 1.47 and terms 1.47 (antipodal_loco single:
# asin next to 1), task rows 1.08 (diff_w_positive_mani_cc all), extras 9.36 (antipodal_mani all: the mean of the orientation reward over 64 envs, where
# the two oracles happen to round alike and the gap is the floor).  lm_post_physics (93 cases): at most 0.45 (terms), obs below 0.005.
# The next power of two above 9.36:
K_TASK = 16
EPS32 = float(np.finfo(np.float32).eps)
GROUPS = ("obs", "states", "rew", "terms", "extras", "task")

EVAL_CASES = [(name, layout, 64) for name in ts.SCENARIOS for layout in ts.LAYOUTS] + \
             [(name, "all", 50) for name in ("knee2_at_loco", "knee3_at_mani", "corner_low_mani", "d23_rst_lo_all4_loco", "d1_pen_hi_beyond_mani", "timeout_and_fall_loco",
                                             "action_clamp_loco_cc", "obs_clip_mani", "rot_decrease_below_then_above_loco_cc", "windows_single_task", "windows_cotrain")]
PHYS_CASES = [(fam, kind, side, layout, 64) for fam in ("loco", "mani", "loco_cc") for kind in ts.PHYS_KINDS for side in (-1, 1) for layout in ("all", "single")] + \
             [(fam, kind, -1, "all", 50) for fam in ("loco", "mani", "loco_cc") for kind in ("knee", "corner", "band_rst")]


@pytest.fixture(scope="module")
def engine_cls():
    from locomanipulationrl_amd.lib import Engine, build_library
    build_library()
    return Engine


def outs(N, num_obs=64):
    return (torch.empty(N, num_obs, device="cuda"), torch.empty(N, 93, device="cuda"), torch.empty(N, device="cuda"),
            torch.empty(N, dtype=torch.int64, device="cuda"), torch.empty(13, device="cuda"))


def ulp_close(a, b):
    """Within one float32 step of the float32 value of b."""
    b32 = np.asarray(b, np.float64).astype(np.float32)
    return bool((np.abs(np.asarray(a, np.float64) - b32.astype(np.float64)) <= np.spacing(np.abs(b32)).astype(np.float64)).all())


def task_rows(ep, task):
    """The float rows of the task state the task layer writes: last tips, goal, and on the PD families the targets and the carried distance."""
    return task[:, 24:40] if ep.variant == 0 else task[:, 24:65] if ep.variant == 1 else task[:, 24:64]


def make_engine(engine_cls, robot_model, blocks, N, split=None, seed=1):
    eng = engine_cls(robot_model, blocks, N, split_env=split if len(blocks) == 2 else None, seed=seed)
    eng.obs_buf, eng.states_buf, eng.terms          # the unclipped views: asked for before anything runs
    return eng


def read_gpu(eng, o):
    torch.cuda.synchronize()
    obs, states, rew, resets, extras = [x.cpu().numpy() for x in o]
    return dict(out_obs=obs.astype(np.float64), out_states=states.astype(np.float64), rew=rew.astype(np.float64), resets=resets, extras=extras.astype(np.float64),
                obs=eng.obs_buf.cpu().numpy().astype(np.float64), states=eng.states_buf.cpu().numpy().astype(np.float64), rew_buf=eng.rew_buf.cpu().numpy().astype(np.float64),
                terms=eng.terms.cpu().numpy().T.astype(np.float64), task32=eng.get_task_env_major(), cnt=eng.get_cnt_env_major(),
                stats=eng.stats_i64.cpu().numpy().copy(), extras_buf=eng.extras_buf.cpu().numpy().astype(np.float64))


def compare(tag, blocks, g, r64, r32, clip_obs=5.0, K=K_TASK):
    """One evaluation: integers and last_actions exactly, on every env; floats per group within K x gap.  Returns the ratios."""
    # ---- integers: the five counters (and the episode number), out_resets, the windows
    assert np.array_equal(g["cnt"], r64["cnt"]), (tag, np.argwhere(g["cnt"] != r64["cnt"])[:8].tolist())
    assert np.array_equal(g["resets"], r64["cnt"][:, 3]), tag
    if "stats" in r64:
        assert np.array_equal(g["stats"][:6], r64["stats"]), (tag, g["stats"][:6], r64["stats"])
        assert ulp_close(g["extras"][7:10], r64["rates"]) and ulp_close(g["extras_buf"][7:10], r64["rates"]), (tag, g["extras"][7:10], r64["rates"])
        if not np.array_equal(g["extras"][7:10].astype(np.float32), np.asarray(r64["rates"], np.float32)):
            print(f"[task branches] {tag}: a published rate one float32 step from the float64 quotient: {g['extras'][7:10]} against {r64['rates']}")
    # ---- last_actions: the clamped actions, bit for bit
    assert np.array_equal(g["task32"][:, 0:12].view(np.int32), r64["task"][:, 0:12].astype(np.float32).view(np.int32)), tag
    assert np.array_equal(g["terms"][:, 7], r64["terms"][:, 7]) and np.array_equal(g["rew"], g["rew_buf"])
    # ---- floats
    assert all(np.isfinite(g[k]).all() for k in ("out_obs", "out_states", "obs", "states", "rew", "terms", "extras"))
    sel = [0, 1, 2, 3, 4, 5, 6, 10, 11, 12]
    ref = lambda r: dict(obs=r["obs"], states=r["states"], rew=r["rew"], terms=r["terms"], extras=r["extras"][sel] if "extras" in r else None,
                         task=np.concatenate([task_rows(b, r["task"][s]).ravel() for b, s in r["_slices"]]))
    a, b = ref(r64), ref(r32)
    gpu = dict(obs=g["obs"], states=g["states"], rew=g["rew"], terms=g["terms"], extras=g["extras"][sel],
               task=np.concatenate([task_rows(bk, g["task32"][s].astype(np.float64)).ravel() for bk, s in r64["_slices"]]))
    ratios = {}
    for grp in GROUPS:
        if a[grp] is None:
            continue
        gap = max(np.abs(a[grp] - b[grp]).max(), 8 * EPS32 * np.abs(a[grp]).max())
        err = np.abs(gpu[grp] - a[grp]).max()
        if grp in ("obs", "states"):          # the returned copies are the clipped ones, the *_buf views are not
            err = max(err, np.abs(g["out_" + grp] - np.clip(a[grp], -clip_obs, clip_obs)).max())
        if grp == "extras":
            err = max(err, np.abs(g["extras_buf"][sel] - a[grp]).max())
        ratios[grp] = err / gap
        print(f"[task branches] {tag}: {grp}: gap {gap:.3e}, max |gpu - f64| {err:.3e}, ratio {ratios[grp]:.2f}")
    for grp, w in ratios.items():
        assert w <= K, (tag, grp, w)
    return ratios


def with_slices(recs, orcs):
    for r in recs:
        r["_slices"] = [(o._ep, sl) for o, sl in orcs]
    return recs


# ------------------------------------------------------------------------------------------------ a. lm_task_eval against the f64 oracle
@pytest.mark.parametrize("name,layout,N", EVAL_CASES)
def test_task_eval_on_the_branch_against_the_oracle(robot_model, engine_cls, name, layout, N):
    """Every scenario x layout through lm_task_eval: no env is left out of any comparison."""
    case = ts.build(name, robot_model, N, 0, layout); blocks = case.blocks
    o64 = ts.oracles(robot_model, case); o32 = ts.oracles(robot_model, case, "f32")
    r64 = with_slices(ts.run(o64, case), o64); r32 = with_slices(ts.run(o32, case), o32)
    eng = make_engine(engine_cls, robot_model, blocks, N, case.split)
    eng.set_task_env_major(case.task); eng.set_cnt_env_major(case.cnt)
    for t in range(case.steps):
        rb, act = case.step(t)
        if case.goal_rand is not None:
            eng.apply_resets(torch.as_tensor(case.goal_rand[t].astype(np.float32), device="cuda"))
        o = outs(N, blocks[0].num_obs)
        eng.task_eval(torch.as_tensor(rb.astype(np.float32), device="cuda").contiguous(), torch.as_tensor(act.astype(np.float32), device="cuda").contiguous(), *o)
        g = read_gpu(eng, o)
        compare(f"{name} {layout} {N} t{t}", blocks, g, r64[t], r32[t])
        # the clamps act on the returned copies alone
        m = ts.layout_mask(N, layout)
        if name.startswith("obs_clip"):
            assert (np.abs(g["out_obs"]) <= 5.0).all() and (np.abs(g["out_states"]) <= 5.0).all()
            assert (np.abs(g["obs"][m]) > 5.0).any(1).all() and (np.abs(g["states"][m]) > 5.0).any(1).all() and (np.abs(g["out_obs"][m]) == 5.0).any(1).all()
        if name.startswith("action_clamp"):
            assert (np.abs(g["task32"][m, 0:12]) == 1.0).all() and (np.abs(g["states"][m, 69:81]) == 1.0).all()
    eng.close()


# ------------------------------------------------------------------------------------------------ b. against the reference's own Python
@pytest.mark.parametrize("name", ts.FIXTURE_SCENARIOS)
def test_task_eval_against_the_reference_on_the_branches(robot_model, engine_cls, name):
    """lm_task_eval on the fixture's own inputs against the fixture's outputs (the reference's Python with the non-zero fall penalty and
    rotation-decrease scale, the short episode and the short window): test_task_layer_against_reference_golden's tolerances."""
    g = np.load(os.path.join(GOLDEN, "task_branches.npz")); N = ts.FIXTURE_N
    ep = ts.build(name, robot_model, N, 0, "all").params; cc = ep.variant == 1
    eng = make_engine(engine_cls, robot_model, [ep], N)
    eng.set_task_env_major(g[f"{name}/task"]); eng.set_cnt_env_major(g[f"{name}/cnt"])
    eng.stats_i64[0:2] = torch.as_tensor(np.array(ts.FIXTURE_STATS0, np.int64), device="cuda")
    for t in range(g[f"{name}/readback"].shape[0]):
        o = outs(N, ep.num_obs); k = f"{name}/{t}/"
        eng.task_eval(torch.as_tensor(g[f"{name}/readback"][t], device="cuda").contiguous(), torch.as_tensor(g[f"{name}/actions"][t], device="cuda").contiguous(), *o)
        torch.cuda.synchronize()
        obs, states, rew, resets, extras = [x.cpu().numpy() for x in o]
        assert np.abs(obs - np.clip(g[k + "obs"], -5, 5)).max() < 2e-5 and np.abs(states - np.clip(g[k + "states"], -5, 5)).max() < 2e-5
        assert np.abs(eng.obs_buf.cpu().numpy() - g[k + "obs"]).max() < 2e-5
        assert np.allclose(rew, g[k + "rew"], rtol=2e-5, atol=1e-4)
        cnt = eng.get_cnt_env_major()
        assert np.array_equal(resets, g[k + "reset_buf"])
        for col, key in enumerate(("successes", "consecutive_successes", "goal_reset_buf", "reset_buf", "progress_buf")):
            assert np.array_equal(cnt[:, col], g[k + key]), (key, t)
        task = eng.get_task_env_major()
        assert np.abs(task[:, 0:12] - g[k + "last_actions"]).max() == 0
        assert np.abs(task[:, 24:36] - g[k + "last_base_tip"]).max() < 2e-6
        if cc:
            assert np.abs(task[:, 40:52] - g[k + "se"]).max() < 2e-6 and np.abs(task[:, 52:64] - g[k + "last_targets"]).max() < 2e-6
        mine = dict(zip(["env/rewards/orientation_rew", "env/rewards/translation_penalty", "env/rewards/joint_acc_penalty", "env/rewards/action_rate_penalty",
                         "env/rewards/consecutive_successes_rew", "env/rewards/joint_limit_panelty", "env/rewards/fall_penalty", "env/success_rate"], extras[:8]))
        mine.update({"env/rewards/mechanical_power_penalty": extras[10], "env/rewards/position_target_error_penalty": extras[11],
                     "env/rewards/rot_dist_decreasing_reward": extras[12]})
        for key, v in zip(g[f"{name}/extras_keys"], g[k + "extras"]):
            assert abs(mine[str(key)] - v) < 2e-5 * max(1.0, abs(v)), (key, t)
        st = eng.stats_i64.cpu().numpy()
        assert st[0] == g[k + "num_successes"] and st[1] == g[k + "num_resets"]
    eng.close()


# ------------------------------------------------------------------------------------------------ c. the step kernels' own instances
@pytest.mark.parametrize("fam,kind,side,layout,N", PHYS_CASES)
def test_post_physics_on_the_branch_against_the_oracle(robot_model, engine_cls, fam, kind, side, layout, N):
    """lm_post_physics (k_step; k_step_pd on the custom-controller family) from physical states: its own kinematics put the lowest knee, one
    corner or the base PHYS_MARGIN to one side of the threshold, or the state carries a joint band, the counter or the timeout case.  The reference
    is built as OracleEngine.post_physics builds it.  Flags exact on every env, floats as in a."""
    from oracle.lmo import Oracle
    ep, phys, act, task, cnt = ts.phys_case(rm := robot_model, N, 0, layout, fam, kind, side)
    recs = []
    for prec in ("f64", "f32"):
        o = Oracle(rm, ep, prec); tk = task.copy()
        r = ts.classify(o, ep, ts.readback_from_phys(o, phys, tk), act, tk, cnt, integrate=False)
        r["task"][:, 12:24] = tk[:, 12:24]; r["_slices"] = [(ep, slice(0, N))]
        ex = np.zeros(13); ex[:7] = r["terms"][:, :7].mean(0); ex[10:13] = r["terms"][:, 8:11].mean(0); r["extras"] = ex
        recs.append(r)
    m = ts.layout_mask(N, layout); fired = recs[0]["flags"][ts._PHYS_FLAG[kind]]; fired = fired.any(1) if fired.ndim == 2 else fired
    assert np.array_equal(fired, m & (side < 0))          # the state is on the side it was built for
    eng = make_engine(engine_cls, rm, [ep], N)
    eng.set_phys_env_major(phys); eng.set_task_env_major(task); eng.set_cnt_env_major(cnt)
    o = outs(N, ep.num_obs); eng.post_physics(torch.as_tensor(act.astype(np.float32), device="cuda").contiguous(), *o)
    g = read_gpu(eng, o)
    compare(f"post_physics {fam} {kind} {side:+d} {layout} {N}", [ep], g, recs[0], recs[1])
    eng.close()


STEP_FAMILIES = {   # name -> (parameter family, environment overrides, engine set-up, the kernel the engine must report)
    "k_step": ("loco", {"LM_H2_MAX_ENVS": "0"}, None, "w1"),
    "k_step_h2": ("loco", {"LM_H2_MAX_ENVS": "1000000"}, None, "h2"),
    "k_step_h3": ("loco", {"LM_H3_MAX_ENVS": "1000000"}, None, "h3"),
    "k_step_w2": ("loco", {"LM_W2_MIN_ENVS": "1"}, None, "w2"),
    "k_step_pd": ("loco_cc", {}, None, "w1"),
    "randomised, all channels off": ("loco_dr", {}, None, "w1"),
    "contact reporting": ("loco", {}, "contact", "w1"),
    "env params": ("loco_dr", {}, "env_params", "w1"),
    "co-training on k_step_h3": ("cotrain", {"LM_H3_MAX_ENVS": "1000000"}, None, "h3"),
}
STEP_CONFIGS = {   # what one step of physics cannot move: the joints barely move (small action scales), the thresholds are far; joint angles are
    # scaled by 10 in the observations, so that the clip_obs clamp acts on the twelve joint-angle rows of every env
    "timeout": dict(max_episode=3, succ_thresh=1.0e-4, max_consec=1, max_reset_counts=30, fall_pen=-50.0, act_scale=0.3, act_scale_se=0.01, s_q=10.0),
    "consecutive successes": dict(max_episode=300, succ_thresh=4.0, max_consec=1, max_reset_counts=30, fall_pen=-50.0, act_scale=0.3, act_scale_se=0.01, s_q=10.0),
}


@pytest.mark.parametrize("config", list(STEP_CONFIGS))
@pytest.mark.parametrize("family", list(STEP_FAMILIES))
def test_step_kernels_own_task_layer_against_oracle_step(robot_model, engine_cls, monkeypatch, family, config):
    """Four lm_step calls at N = 50 on each kernel family against Oracle.step (OracleEngine): timeouts with max_episode = 3, consecutive-success
    resets with succ_thresh = 4 (every pose is a success), a window of 30 resets that rolls on the way, actions of up to +-1.5 that the clamp cuts.
    Counters, reset flags, windows and published rates equal after every step, on every env; the bonus and fall-penalty means follow.  The
    returned observations and states are the engine's own unclipped views clamped to +-clip_obs, bit for bit, and the clamp acts in every env (on
    k_step_h3 the full wavefronts leave through the helper wavefront's copy of the clamp, the ragged last one through write_outputs')."""
    from locomanipulationrl_amd.engine_config import loco_cc_params, loco_params, mani_params
    fam, env, setup, variant = STEP_FAMILIES[family]; kw = STEP_CONFIGS[config]; N = 50
    blocks = {"loco": [loco_params(**kw)], "loco_cc": [loco_cc_params(**kw)], "loco_dr": [loco_params(dr_enabled=1, **kw)],
              "cotrain": [loco_params(**kw), mani_params(**kw)]}[fam]
    split = 32 if fam == "cotrain" else None
    for k in ("LM_H2_MAX_ENVS", "LM_H3_MAX_ENVS", "LM_W2_MIN_ENVS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = make_engine(engine_cls, robot_model, blocks, N, split, seed=42)
    for k in env:
        monkeypatch.delenv(k)
    if setup == "contact":
        eng.enable_contact_forces(True)
    if setup == "env_params":
        eng.enable_env_params()
    assert eng.step_variant == variant
    oe = OracleEngine(robot_model, blocks, N, split, 42, 5.0, 1.0)
    eng.reset_all(); oe.reset_all()
    rng = np.random.default_rng(11); seen = dict(timeout=0, goal=0, rolled=0)
    for t in range(4):
        act = rng.uniform(-1.5, 1.5, size=(N, 12)).astype(np.float32)
        before = oe.stats_i64.numpy().copy()
        oe.step(torch.as_tensor(act))
        o = outs(N, blocks[0].num_obs); eng.step(torch.as_tensor(act, device="cuda"), None, *o); torch.cuda.synchronize()
        cnt = eng.get_cnt_env_major(); want = oe.cntv
        assert np.array_equal(cnt, want), (family, config, t, np.argwhere(cnt != want)[:8].tolist())
        assert np.array_equal(o[3].cpu().numpy(), want[:, 3])
        assert np.array_equal(eng.stats_i64.cpu().numpy()[:6], oe.stats_i64.numpy()), (family, config, t)
        ex = o[4].cpu().numpy(); oex = oe.extras_buf.numpy()
        assert ulp_close(ex[7:10], oex[7:10].astype(np.float64)), (ex[7:10], oex[7:10])
        assert np.array_equal(eng.get_task_env_major()[:, 0:12].view(np.int32), np.clip(act, -1, 1).view(np.int32))
        assert abs(ex[4] - oex[4]) <= 1e-5 * max(1.0, abs(oex[4])) and abs(ex[6] - oex[6]) <= 1e-5 * max(1.0, abs(oex[6]))
        for out, view, ref in ((o[0], eng.obs_buf, oe.obs_buf), (o[1], eng.states_buf, oe.states_buf)):
            assert torch.equal(out, view.clamp(-5.0, 5.0)) and bool((view.abs() > 5.0).any(1).all()) and float(out.abs().max()) == 5.0
            assert bool(((view.cpu().abs() > 5.0) == (ref.abs() > 5.0)).all())          # the same elements as on the oracle
        seen["timeout"] += int((want[:, 3] == 1).sum()) if config == "timeout" else 0
        seen["goal"] += int(want[:, 2].sum()); seen["rolled"] += int((oe.stats_i64.numpy()[1] < before[1]))
    assert seen["rolled"] >= 1 and (seen["timeout"] >= N if config == "timeout" else seen["goal"] >= N), seen
    eng.close()
