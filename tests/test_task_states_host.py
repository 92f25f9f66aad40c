"""CPU checks of tests/task_states.py, the conditions test_gpu_task_branches.py stands on:
  - every scenario x layout takes its branch on the envs of the layout - on limb limb_of(env) alone where the cause is per limb - and on no other
    env, and a case that must not fire sits within its stated distance of the threshold (0: exactly on it);
  - the float32 oracle classifies every env, and every limb, as the float64 oracle does: zero disagreements, a condition on the inputs;
  - the float64 oracle reproduces tests/golden/task_branches.npz, the reference's own Python on the scenarios the eleven task_*.npz files are blind
    to (non-zero fall penalty and rotation-decrease scale, short episodes, a short success-rate window), to test_oracle_golden.py's tolerances."""
import os

import numpy as np
import pytest

import task_states as ts
from conftest import GOLDEN
from oracle.lmo import Oracle

CASES = [(name, layout) for name in ts.SCENARIOS for layout in ts.LAYOUTS]
N = 64


@pytest.fixture(scope="module")
def ran(robot_model):
    """(case, float64 records, float32 records) per scenario x layout x N, computed once."""
    cache = {}

    def get(name, layout, n=N):
        key = (name, layout, n)
        if key not in cache:
            case = ts.build(name, robot_model, n, 0, layout)
            cache[key] = (case, ts.run(ts.oracles(robot_model, case), case), ts.run(ts.oracles(robot_model, case, "f32"), case))
        return cache[key]
    return get


def test_inputs_are_float32_values(robot_model):
    for name in ("knee2_at_mani", "rot_decrease_above_then_below_loco_cc", "windows_cotrain"):
        case = ts.build(name, robot_model, 32, 0, "alternate")
        for a in (case.readback, case.actions, case.task):
            assert np.array_equal(a, a.astype(np.float32).astype(np.float64))
        assert case.cnt.dtype == np.int64


def test_limb_of_covers_the_quad_under_every_layout():
    for layout in ts.LAYOUTS:
        assert set(ts.limb_of(np.arange(64))[ts.layout_mask(64, layout)].tolist()) == {0, 1, 2, 3}, layout
    assert ts.limb_of(np.array([0, 17, 34, 51])).tolist() == [0, 1, 2, 3]


@pytest.mark.parametrize("name,layout", CASES)
def test_branch_is_taken_on_the_layout_and_nowhere_else(ran, name, layout):
    case, r64, _ = ran(name, layout); sc = ts.SCENARIOS[name]; m = ts.layout_mask(N, layout)
    if sc["flag"] is None:
        return
    rec = r64[sc["step"]]; f = rec["flags"][sc["flag"]]
    want = m if f.ndim == 1 else m[:, None] & ts._one_limb(N, sc["all4"])
    if sc["flag"] == "rdec_gate":          # a gate with two open sides: the nominal envs (0.5-0.9 rad) are above it
        assert np.array_equal(f[m], np.full(int(m.sum()), sc["fires"])) and f[~m].all()
    elif sc["fires"]:
        assert np.array_equal(f, want), (name, layout, int(f.sum()), int(want.sum()))
    else:
        assert not f.any(), (name, layout)
        if sc["edge"] is not None:          # ... although it sits on (or next to) the threshold
            assert (np.abs(rec["dist"]["d_" + sc["flag"]][want]) <= sc["edge"]).all(), np.abs(rec["dist"]["d_" + sc["flag"]][want]).max()
    # the nominal envs are clear of everything: no success, no reset, no penalty band, no clamp
    for k in ("success", "reset", "limit_pen", "charged", "bonus", "act_clamped", "obs_clipped", "states_clipped", "se_lo", "se_hi"):
        assert not rec["flags"][k][~m].any(), (name, layout, k)


@pytest.mark.parametrize("name,layout", CASES)
def test_float32_oracle_classifies_every_env_like_the_float64_oracle(ran, name, layout):
    """Zero disagreements over every flag, counter and window of every evaluation: a condition on the inputs (widen a margin, never drop an env)."""
    _, r64, r32 = ran(name, layout)
    for t, (a, b) in enumerate(zip(r64, r32)):
        for k in ts.FLAG_NAMES:
            assert np.array_equal(a["flags"][k], b["flags"][k]), (name, layout, t, k, int((a["flags"][k] != b["flags"][k]).sum()))
        assert np.array_equal(a["cnt"], b["cnt"]) and np.array_equal(a["stats"], b["stats"]) and a["rolled"] == b["rolled"]
        assert np.array_equal(a["task"][:, 0:12], b["task"][:, 0:12])          # last_actions: the clamped actions themselves


@pytest.mark.parametrize("layout", ts.LAYOUTS)
@pytest.mark.parametrize("fam", ["loco", "mani"])
def test_counter_machine_and_bonus(ran, fam, layout):
    m = ts.layout_mask(N, layout); mc = ts.EXACT["max_consec"]
    for (b, n), consec_after in (((0, 0), 0), ((0, 1), 1), ((1, 0), 0), ((1, 1), 2 * 1 + 1)):
        rec = ran(f"counters_{b}{n}_{fam}", layout)[1][0]
        assert (rec["cnt"][m, 0] == n).all() and (rec["cnt"][m, 1] == consec_after).all() and not rec["flags"]["bonus"].any()
    for k, c in (("below", mc - 1), ("at", mc), ("beyond", mc + 1)):
        rec = ran(f"consec_{k}_{fam}", layout)[1][0]; hit = m if k == "beyond" else np.zeros(N, bool)
        assert (rec["cnt"][m, 1] == c + 1).all()
        for flag in ("bonus", "goal_reset", "reset"):
            assert np.array_equal(rec["flags"][flag], hit), (k, flag)
        assert np.array_equal(rec["terms"][:, 4] == 600.0, hit) and not rec["flags"]["charged"].any()          # the goal reset is not charged


@pytest.mark.parametrize("fam", ["loco", "mani"])
def test_fall_penalty_ordering_and_timeout(ran, fam):
    m = ts.layout_mask(N, "alternate")
    rec = ran(f"carried_reset_{fam}", "alternate")[1][0]
    assert np.array_equal(rec["terms"][:, 6] == -50.0, m) and np.array_equal(rec["flags"]["reset"], m)
    for left, fires in ((3, False), (2, True), (1, True)):
        rec = ran(f"timeout_{left}_{fam}", "alternate")[1][0]
        assert np.array_equal(rec["flags"]["reset"], m & fires) and not rec["flags"]["charged"].any() and (rec["terms"][:, 6] == 0).all()
    rec = ran(f"timeout_and_fall_{fam}", "alternate")[1][0]
    assert np.array_equal(rec["terms"][:, 6] == -50.0, m) and (rec["terms"][~m, 6] == 0).all() and np.array_equal(rec["flags"]["timeout"], m)
    rew_nofall = ran(f"timeout_1_{fam}", "alternate")[1][0]["rew"]
    assert np.abs(rec["rew"][m] - (rew_nofall[m] - 50.0)).max() < 1e-9          # charged once


@pytest.mark.parametrize("fam", ["loco", "mani"])
def test_quaternion_edges(ran, fam):
    m = ts.layout_mask(N, "single")
    case, r64, r32 = ran(f"antipodal_{fam}", "single")
    for r in (r64[0], r32[0]):
        assert np.isfinite(r["rew"]).all() and np.abs(r["rot_dist"][m] - np.pi).max() < 2e-3
    rec = ran(f"identity_diff_{fam}", "single")[1][0]
    assert (rec["rot_dist"][m] == 0).all() and (rec["terms"][m, 0] == 0.5 / 0.1).all()


@pytest.mark.parametrize("fam", ["loco", "loco_cc", "loco_pc", "mani", "mani_cc"])
def test_difference_quaternion_flips_except_on_the_custom_controller_family(ran, fam):
    m = ts.layout_mask(N, "alternate")
    neg = ran(f"diff_w_negative_{fam}", "alternate")[1][0]; pos = ran(f"diff_w_positive_{fam}", "alternate")[1][0]
    assert np.abs(pos["obs"][m, 6] - 0.01).max() < 1e-6
    assert np.abs(neg["obs"][m, 6] - (-0.01 if fam.endswith("_cc") else 0.01)).max() < 1e-6
    assert np.abs(neg["states"][m, 41] - neg["obs"][m, 6]).max() == 0
    if fam.startswith("mani"):
        for w in ("negative", "positive"):
            rec = ran(f"plate_w_{w}_{fam}", "alternate")[1][0]
            case = ran(f"plate_w_{w}_{fam}", "alternate")[0]; raw = ts.qmul(np.tile(ts.qconj(ts.FLIP), (N, 1)), case.readback[:, 39:43])[:, 0]
            assert (raw[m] < 0).all() if w == "negative" else (raw[m] > 0).all()
            # oq.w is flipped to the positive side: 0.01 x cos(tilt / 2), tilt <= 0.08 rad
            assert np.abs(rec["states"][m, 6] - 0.01).max() < 1e-5 and (rec["states"][:, 6] > 0).all() and not rec["flags"]["reset"].any()


@pytest.mark.parametrize("fam", ["loco", "mani", "loco_cc"])
def test_clamps_act_on_the_right_copy(ran, fam):
    m = ts.layout_mask(N, "alternate")
    case, r64, _ = ran(f"action_clamp_{fam}", "alternate"); rec = r64[0]
    assert (np.abs(case.actions[m]) == 1.5).all() and (np.abs(rec["task"][m, 0:12]) == 1.0).all() and (np.abs(rec["states"][m, 69:81]) == 1.0).all()
    if fam != "loco_pc":
        assert (np.abs(rec["obs"][m, 40:52]) == 1.0).all()
    rec = ran(f"obs_clip_{fam}", "alternate")[1][0]
    assert (np.abs(rec["obs"][m, 28:40]) > 5.0).all() and (np.abs(rec["obs"][m][:, [12, 15]]) > 5.0).all() and (np.abs(rec["states"][m, 25:37]) > 5.0).all()
    assert (np.abs(rec["obs"][m, 0:2]) > 5.0).any(1).all() and (np.abs(rec["states"][m][:, [5, 12]]) > 5.0).all()


@pytest.mark.parametrize("fam", ["loco_cc", "mani_cc"])
def test_rotation_decrease_term_reads_the_carried_distance(ran, fam):
    m = ts.layout_mask(N, "all")
    for name, gates in ((f"rot_decrease_above_then_below_{fam}", (True, False)), (f"rot_decrease_below_then_above_{fam}", (False, True))):
        case, r64, _ = ran(name, "all"); th = case.params.rot_dec_thresh
        assert np.array_equal(r64[0]["flags"]["rdec_gate"], m & gates[0]) and np.array_equal(r64[1]["flags"]["rdec_gate"], m & gates[1])
        want0 = np.where(gates[0], (0.9 - r64[0]["rot_dist"]) * 2.0, 0.0); want1 = np.where(gates[1], (r64[0]["rot_dist"] - r64[1]["rot_dist"]) * 2.0, 0.0)
        assert np.abs(r64[0]["terms"][:, 10] - want0).max() < 1e-6 and np.abs(r64[1]["terms"][:, 10] - want1).max() < 1e-6
        assert np.abs(np.abs(want0) + np.abs(want1)).min() > 0.2          # the term is there: 0.1 or 0.15 rad x 2 at the least
        assert np.abs(r64[1]["task"][:, 64] - r64[1]["rot_dist"]).max() < 1e-9
    a = ran(f"last_targets_update_0_{fam}", "all")[1]; b = ran(f"last_targets_update_1_{fam}", "all")[1]
    assert np.abs(a[0]["terms"][:, 9] - b[0]["terms"][:, 9]).max() == 0 and np.abs(a[1]["terms"][:, 9] - b[1]["terms"][:, 9]).min() > 1e-4
    assert (a[1]["task"][:, 52:64] == a[0]["task"][:, 52:64]).all() and (b[1]["task"][:, 52:64] != b[0]["task"][:, 52:64]).any()


@pytest.mark.parametrize("layout", ts.LAYOUTS)
@pytest.mark.parametrize("name", ["windows_single_task", "windows_cotrain"])
@pytest.mark.parametrize("n", [64, 50])
def test_windows_roll_inside_six_evaluations_and_not_together(ran, name, layout, n):
    case, r64, _ = ran(name, layout, n)
    assert case.steps == ts.T_WINDOWS and case.split % 16 == 0
    rolled = np.array([r["rolled"] for r in r64])          # [T][3]
    if name == "windows_single_task":          # one block: the first-task window is the all-envs window, the second-task one stays empty
        assert rolled[:, 0].any() and np.array_equal(rolled[:, 0], rolled[:, 1]) and not rolled[:, 2].any() and (r64[-1]["stats"][4:6] == 0).all()
    else:
        assert rolled.any(0).all(), rolled
        first = [int(np.argmax(rolled[:, w])) for w in range(3)]
        assert len(set(first)) > 1, first
    assert max(r["rates"].max() for r in r64) > 0          # a published rate that is not the initial zero
    for r in r64:
        assert r["stats"][0] <= r["stats"][1] and (r["stats"] >= 0).all()
    halves = [(int(r["cnt"][:case.split, 3].sum()), int(r["cnt"][case.split:, 3].sum())) for r in r64]
    assert [a for a, _ in halves] != [b for _, b in halves]          # the two halves reset on different evaluations


@pytest.mark.parametrize("fam", ["loco", "mani", "loco_cc"])
@pytest.mark.parametrize("kind", ts.PHYS_KINDS)
def test_physical_states_sit_on_their_side_in_both_precisions(robot_model, fam, kind):
    """The states of lm_post_physics' test: the oracle's kinematics put the knee, the corner or the base at least 1e-3 m (PHYS_MARGIN = 2e-3) to
    the side the case names, on the layout's envs alone, and the float32 oracle agrees on every flag of every env."""
    for side in (-1, 1):
        for layout in ts.LAYOUTS:
            for n in (64, 50):
                ep, phys, act, task, cnt = ts.phys_case(robot_model, n, 0, layout, fam, kind, side); m = ts.layout_mask(n, layout); recs = []
                for prec in ("f64", "f32"):
                    o = Oracle(robot_model, ep, prec); tk = task.copy()
                    recs.append(ts.classify(o, ep, ts.readback_from_phys(o, phys, tk), act, tk, cnt, integrate=False))
                for k in ts.FLAG_NAMES:
                    assert np.array_equal(recs[0]["flags"][k], recs[1]["flags"][k]), (side, layout, n, k)
                flag = ts._PHYS_FLAG[kind]; f = recs[0]["flags"][flag]; f = f.any(1) if f.ndim == 2 else f
                assert np.array_equal(f, m & (side < 0)), (side, layout, n)
                assert np.array_equal(recs[0]["flags"]["reset"], m & (side < 0) & (kind != "band_pen"))
                if kind in ("knee", "corner", "base"):
                    d = recs[0]["dist"]["d_" + flag]; d = d if d.ndim == 1 else d[np.arange(n), ts.limb_of(np.arange(n))]
                    assert (np.abs(d[m] - side * ts.PHYS_MARGIN) < 1e-5).all() and (np.abs(d) >= 1e-3).all()


# ------------------------------------------------------------------------------------------------ the fixture
EXTRAS_TO_TERM = {"env/rewards/action_rate_penalty": 3, "env/rewards/consecutive_successes_rew": 4, "env/rewards/fall_penalty": 6,
                  "env/rewards/joint_acc_penalty": 2, "env/rewards/joint_limit_panelty": 5, "env/rewards/orientation_rew": 0,
                  "env/rewards/translation_penalty": 1, "env/rewards/mechanical_power_penalty": 8,
                  "env/rewards/position_target_error_penalty": 9, "env/rewards/rot_dist_decreasing_reward": 10}


def check_against_fixture(g, name, recs, obs_tol=2e-6, rew_tol=(1e-5, 5e-5), extras_rel=1e-5):
    """Per-evaluation records (classify()'s keys, plus stats / rates where the fixture has them) against the reference's own Python."""
    for t, r in enumerate(recs):
        k = f"{name}/{t}/"
        assert np.abs(r["obs"] - g[k + "obs"]).max() < obs_tol and np.abs(r["states"] - g[k + "states"]).max() < obs_tol
        assert np.allclose(r["rew"], g[k + "rew"], rtol=rew_tol[0], atol=rew_tol[1])
        for col, key in enumerate(("successes", "consecutive_successes", "goal_reset_buf", "reset_buf", "progress_buf")):
            assert np.array_equal(r["cnt"][:, col], g[k + key]), (name, t, key)
        assert np.abs(r["task"][:, 0:12] - g[k + "last_actions"]).max() == 0
        assert np.abs(r["task"][:, 24:36] - g[k + "last_base_tip"]).max() < obs_tol
        if k + "last_targets" in g:
            assert np.abs(r["task"][:, 52:64] - g[k + "last_targets"]).max() < obs_tol and np.abs(r["task"][:, 64] - g[k + "last_rot_dist"]).max() < 10 * obs_tol
        for key, v in zip(g[f"{name}/extras_keys"], g[k + "extras"]):
            if str(key) in EXTRAS_TO_TERM:
                assert abs(r["terms"][:, EXTRAS_TO_TERM[str(key)]].mean() - v) < extras_rel * max(1, abs(v)), (name, t, key)
        assert r["stats"][0] == g[k + "num_successes"] and r["stats"][1] == g[k + "num_resets"]
        assert abs(r["rates"][0] - g[k + "success_rate"]) < 1e-6


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "task_branches.npz"))


def test_fixture_holds_what_it_should(fixture):
    assert os.path.getsize(os.path.join(GOLDEN, "task_branches.npz")) <= max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN)
                                                                             if f.startswith("task_") and f != "task_branches.npz")
    assert sorted(str(n) for n in fixture["names"]) == sorted(ts.FIXTURE_SCENARIOS)
    assert os.path.getsize(os.path.join(GOLDEN, "task_branches.npz")) <= 1 << 20
    charged = sum(float((fixture[f"{n}/0/extras"][list(fixture[f"{n}/extras_keys"]).index("env/rewards/fall_penalty")] != 0)) for n in ts.FIXTURE_SCENARIOS)
    assert charged >= 14          # the fall penalty is there: seven causes on two families at the least


@pytest.mark.parametrize("name", ts.FIXTURE_SCENARIOS)
def test_float64_oracle_reproduces_the_reference_on_the_branches(robot_model, fixture, name):
    """The scenario is built again here (same seed, N = 16, `all`); the fixture's own copy of the inputs must be the same bits, then the oracle's
    outputs are the reference's to test_oracle_golden.py's tolerances, windows and published rate included."""
    case = ts.build(name, robot_model, ts.FIXTURE_N, 0, "all"); g = fixture
    assert np.array_equal(np.asarray(case.readback, np.float32).reshape(case.steps, ts.FIXTURE_N, 99), g[f"{name}/readback"])
    assert np.array_equal(case.task.astype(np.float32), g[f"{name}/task"]) and np.array_equal(case.cnt, g[f"{name}/cnt"])
    assert np.array_equal(np.asarray(case.actions, np.float32).reshape(case.steps, ts.FIXTURE_N, 12), g[f"{name}/actions"])
    check_against_fixture(g, name, ts.run(ts.oracles(robot_model, case), case, stats0=ts.FIXTURE_STATS0))
