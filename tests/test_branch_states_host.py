"""The branch-point states of tests/branch_states.py on the CPU: every scenario x layout really takes the branch it is named after (and the
nominal envs next to it do not), and the reference itself is well behaved there - the float32 and float64 oracles take the same branches on
every foot and joint and differ by less than the one-sub-step contract of test_gpu_parity.py.  A GPU miss on these states is then the
kernel's, not the recipe's.

MIN_SHARE: the share of feet / joints of the branch envs that must carry the scenario's flag, about half of what the float64 oracle gives
for the recipe at 64 envs, seed 0 (measured: speed limit 0.14, torque limit 0.37 / 0.73 on the plate scene, capped bias 0.62, off the plate
0.50 in x and 0.27 in y, loaded at a large tilt 0.22, speculative 0.53)."""
import numpy as np
import pytest

import branch_states as bs
from oracle.lmo import Oracle

MIN_SHARE = {"speed_limit": 0.06, "torque_limit": 0.18, "torque_limit_mani": 0.36, "depenetration_cap": 0.30, "plate_rim_x": 0.25,
             "plate_rim_y": 0.12, "large_tilt_contact": 0.11, "speculative_gap": 0.26}
CASES = [(name, layout, 64) for name in bs.SCENARIOS for layout in bs.LAYOUTS] + [(name, "all", 50) for name in bs.SCENARIOS]
FOOT_FLAGS, JOINT_FLAGS = ("loaded", "off_plate", "capped"), ("torque_limit", "speed_limit")


@pytest.fixture(scope="module")
def classified(robot_model):
    """(ep, phys, targets, f64 classification, f32 classification) per case, computed once."""
    cache = {}

    def get(name, layout, N):
        key = (name, layout, N)
        if key not in cache:
            ep, phys, tg = bs.build(name, robot_model, N, 0, layout)
            c64 = bs.classify(Oracle(robot_model, ep), ep, phys, tg)
            c32 = bs.classify(Oracle(robot_model, ep, precision="f32"), ep, phys, tg)
            cache[key] = (ep, phys, tg, c64, c32)
        return cache[key]
    return get


def test_layouts():
    assert bs.layout_mask(64, "all").all() and bs.layout_mask(64, "alternate").sum() == 32
    assert np.flatnonzero(bs.layout_mask(64, "single")).tolist() == [0, 17, 34, 51]
    assert np.flatnonzero(bs.layout_mask(50, "single")).tolist() == [0, 17, 34]


@pytest.mark.parametrize("name,layout,N", CASES)
def test_states_are_float32_values_with_unit_quaternions(classified, name, layout, N):
    ep, phys, tg, _, _ = classified(name, layout, N)
    assert phys.shape == (N, 50) and tg.shape == (N, 12) and phys.dtype == np.float64
    assert np.array_equal(phys, phys.astype(np.float32).astype(np.float64)) and np.array_equal(tg, tg.astype(np.float32).astype(np.float64))
    for s in (3, 40):
        assert np.abs(np.linalg.norm(phys[:, s:s + 4], axis=1) - 1).max() < 2e-7


@pytest.mark.parametrize("name,layout,N", CASES)
def test_the_branch_is_taken_where_the_layout_says(classified, name, layout, N):
    ep, phys, tg, c, _ = classified(name, layout, N)
    m = bs.layout_mask(N, layout); flag = bs.SCENARIOS[name][1]
    if name == "stick_and_slide":
        ld = c["loaded"][m].sum()
        print(f"[branch states] {name} {layout} {N}: loaded {c['loaded'][m].mean():.2f}, stick {c['stick'][m].sum() / ld:.2f}, slide {c['slide'][m].sum() / ld:.2f} of the loaded feet")
        assert c["loaded"][m].mean() >= 0.25
        assert c["stick"][m].sum() >= 0.10 * ld and c["slide"][m].sum() >= 0.10 * ld
        assert not c["loaded"][~m].any()
    elif name == "zero_spin_free_fall":
        # the free body's angular velocity is exactly zero before and after the sub-step (th == 0); the nominal envs' plates turn
        assert (phys[m, 47:50] == 0).all() and (c["post"][m, 47:50] == 0).all() and not c["loaded"][m].any()
        assert (np.abs(c["post"][~m, 47:50]).max(1) > 1e-3).all()
        assert np.array_equal(c["post"][m, 40:44], phys[m, 40:44]) and np.array_equal(c["post"][m, 37:39], phys[m, 37:39])
        assert (c["post"][m, 39] < phys[m, 39]).all()
    else:
        share = c[flag][m].mean()
        print(f"[branch states] {name} {layout} {N}: {flag} on {share:.2f} of the branch envs' feet / joints")
        assert share >= MIN_SHARE[name], (share, MIN_SHARE[name])
        assert not c[flag][~m].any(), "a nominal env took the branch"
    if name.startswith("plate_rim"):
        both = c["off_plate"].any(1) & (c["loaded"] & ~c["off_plate"]).any(1)
        print(f"[branch states] {name} {layout} {N}: {both[m].mean():.2f} of the branch envs have feet off the plate next to loaded feet on it")
        assert both[m].mean() >= 0.25
        assert not (c["loaded"] & c["off_plate"]).any()
    if name == "large_tilt_contact":
        assert c["loaded"][m].any(1).mean() >= 0.6          # most tilted envs stand on at least one foot
    if name == "depenetration_cap":
        assert (c["capped"] <= c["penetrating"]).all() and (c["capped"] & c["loaded"])[m].mean() >= 0.25
    if name == "speculative_gap":
        assert not c["penetrating"][m].any()          # every foot starts above the surface


def test_large_tilt_really_is_large(robot_model):
    ep, phys, tg = bs.build("large_tilt_contact", robot_model, 64, 0, "all")
    q = phys[:, 3:7]; zz = 1 - 2 * (q[:, 1] ** 2 + q[:, 2] ** 2)          # cos of the angle between the base's z axis and the vertical
    tilt = np.arccos(np.clip(zz, -1, 1))
    assert tilt.min() > 0.49 and tilt.max() < 1.21


@pytest.mark.parametrize("name,layout,N", CASES)
def test_the_reference_takes_the_same_branches_in_both_precisions(classified, name, layout, N):
    ep, phys, tg, c64, c32 = classified(name, layout, N)
    for k in FOOT_FLAGS + JOINT_FLAGS:
        assert np.array_equal(c64[k], c32[k]), (k, int((c64[k] != c32[k]).sum()))
    ge = bs.group_errors(ep, c32["post"], c64["post"])
    print(f"[branch states] {name} {layout} {N}: f32 - f64 / contract " + ", ".join(f"{g} {v.max() / bs.CONTRACT[g]:.3f}" for g, v in ge.items()))
    for g, v in ge.items():
        assert v.max() <= bs.CONTRACT[g], (g, v.max())


@pytest.mark.parametrize("name,layout,N", CASES)
def test_four_substeps_stay_finite(robot_model, classified, name, layout, N):
    ep, phys, tg, _, _ = classified(name, layout, N)
    o = Oracle(robot_model, ep); p = phys.copy()
    for _ in range(4):
        o.substep(p, tg)
    assert np.isfinite(p).all() and np.abs(np.linalg.norm(p[:, 3:7], axis=1) - 1).max() < 1e-9


@pytest.mark.parametrize("name", ["torque_limit", "speed_limit"])
def test_randomised_limits_separate_from_the_nominal_ones(robot_model, name):
    """The negative control of the GPU test of k_step_dr, on the CPU first: one control step with per-env draws of the torque and speed limits
    against the same step with the nominal limits (both float64) differs in the observations by far more than 100 x what the float32 oracle
    differs from the float64 one with the same draws."""
    N = 32
    ep0, phys, tg = bs.build(name, robot_model, N, 0, "all")
    sc = float(np.ceil(np.abs(tg).max())); ep, ep_nom = bs.randomised_limits(sc); act = tg / sc
    obs = {}
    for key, e, prec in (("dr64", ep, "f64"), ("dr32", ep, "f32"), ("nom64", ep_nom, "f64")):
        o = Oracle(robot_model, e, precision=prec); p, task, cnt = o.new_state(N); o.reset(p, task, cnt, seed=21); p[:] = phys
        if e.dr_enabled:
            res = o.step_dr(p, task, cnt, o.new_dr_counters(N), act.astype(o.dtype), clip_actions=1.0, seed=21)
            assert res[5][:, :12].min() < 0.9 and res[5][:, :12].max() > 2.0 and res[5][:, 12:24].min() < 4.0 and res[5][:, 12:24].max() > 7.0
        else:
            res = o.step(p, task, cnt, act.astype(o.dtype), seed=21)
        obs[key] = np.clip(res[0], -5, 5).astype(np.float64)
    parity = np.abs(obs["dr32"] - obs["dr64"]).max(1); control = np.abs(obs["nom64"] - obs["dr64"]).max(1)
    print(f"[branch states] randomised limits from {name}: f32 - f64 median {np.median(parity):.2e} max {parity.max():.2e}; nominal limits median {np.median(control):.2e}")
    assert parity.max() < 5e-3 and np.median(control) > 1e-2 and np.median(control) >= 100 * max(np.median(parity), 1e-4)
