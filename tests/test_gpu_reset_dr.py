"""Reset-state randomisation on the MI355X: k_step_dr / k_step_dr_pd draw the state an env is reset to (joint positions and
velocities, the free body's position and orientation) inside the step launch, at every reset that passes the min_frequency gate, and record it
in Engine.dr_reset_state.  The expected draws are arithmetic on the oracle's `dr_sample` (tests/reset_dr_reference.py); the oracle itself knows
nothing of reset randomisation."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import reset_dr_reference as R
from locomanipulationrl_amd.engine_config import (DR_RESET_JOINT_POS, DR_RESET_JOINT_VEL, DR_RESET_ORIENTATION, DR_RESET_POSITION, DRChannel, loco_cc_params,
                                                  loco_params, mani_cc_params, mani_params)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine_cls():
    from locomanipulationrl_amd.lib import Engine, build_library
    build_library()
    return Engine


@pytest.fixture(scope="module")
def oracle_cls():
    from oracle.lmo import Oracle
    return Oracle


def outs(N, num_obs=64):
    return (torch.empty(N, num_obs, device="cuda"), torch.empty(N, 93, device="cuda"), torch.empty(N, device="cuda"),
            torch.empty(N, dtype=torch.int64, device="cuda"), torch.empty(13, device="cuda"))


def randomised(make, channels=None, min_frequency=0, **kw):
    return make(dr_enabled=1, dr_min_frequency=min_frequency, dr_reset=R.reference_channels() if channels is None else channels, **kw)


def actions(N, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand(N, 12, device="cuda", generator=g) * 2 - 1


# every operation a channel accepts and every distribution: [joint_positions, joint_velocities, position, orientation]
DRAW_CASES = {
    "reference": R.reference_channels,
    "scaling_direct": lambda: [R.chan("scaling", "loguniform", 0.95, 1.05), R.chan("direct", "gaussian", 0.0, 0.05),
                               R.chan("scaling", "uniform", [0.9, 0.9, 0.9], [1.1, 1.1, 1.5]), R.chan("direct", "gaussian", [0.0, 0.0, 0.3], [0.05, 0.05, 0.5])],
    "direct_additive": lambda: [R.chan("direct", "gaussian", 0.2, 0.1), R.chan("additive", "loguniform", 0.01, 0.1),
                                R.chan("direct", "uniform", [-0.05, -0.05, 0.14], [0.05, 0.05, 0.24]), R.chan("additive", "gaussian", [0.0, 0.0, 0.0], [0.05, 0.05, 0.6])],
    "additive_loguniform": lambda: [R.chan("additive", "gaussian", 0.0, 0.05), R.chan("direct", "uniform", -0.1, 0.1),
                                    R.chan("additive", "loguniform", [0.001, 0.001, 0.001], [0.05, 0.05, 0.1]), R.chan("direct", "loguniform", [0.01, 0.01, 0.1], [0.1, 0.1, 1.2])],
}
DRAW_BLOCKS = {"loco": loco_params, "mani": mani_params, "loco_cc": loco_cc_params, "mani_cc": mani_cc_params}


@pytest.mark.parametrize("case", list(DRAW_CASES))
@pytest.mark.parametrize("block", list(DRAW_BLOCKS))
def test_draws_match_the_oracle_samples(robot_model, engine_cls, oracle_cls, block, case):
    """256 envs, min_frequency 0, every env flagged: after one step dr_reset_state is operation(nominal, dr_sample(seed, stream, env, episode 1,
    component)).  Tolerance: that of test_domain_randomisation_step_parity for sampled attributes, 2e-5 per unit of magnitude (fp32 rounding of
    the log / cos inside dr_sample); the stored quaternion is unit length within 1e-6."""
    N, seed = 256, 77
    ep = randomised(DRAW_BLOCKS[block], DRAW_CASES[case]())
    eng = engine_cls(robot_model, [ep], N, seed=seed)
    eng.step(actions(N, 1), None, *outs(N, ep.num_obs)); torch.cuda.synchronize()
    got = eng.dr_reset_state.cpu().numpy().T.astype(np.float64)
    exp = R.expected_state(oracle_cls(robot_model, ep), ep, seed, np.arange(N), np.ones(N, np.int64))
    err = np.abs(got - exp) / np.maximum(1.0, np.abs(exp))
    print(f"{block}/{case}: largest error per unit of magnitude {err.max():.3e}; |quat| - 1 {np.abs(np.linalg.norm(got[:, 27:31], axis=1) - 1).max():.3e}")
    assert err.max() < 2e-5, (err.max(), np.unravel_index(err.argmax(), err.shape))
    assert np.abs(np.linalg.norm(got[:, 27:31], axis=1) - 1).max() < 1e-6
    moved = np.abs(exp - R.nominal_state(ep)).max(0)
    assert np.delete(moved, [24, 25]).min() > 1e-3          # every component was really drawn (x, y: nominal 0, which `scaling` leaves at 0)
    eng.close()


def test_draws_on_a_cotraining_engine(robot_model, engine_cls, oracle_cls):
    """Two blocks, one launch: each half uses its own block's channels and nominal state; the stream is keyed by the global env id."""
    N, seed = 64, 5
    lo = randomised(loco_params); ma = randomised(mani_params, DRAW_CASES["scaling_direct"]())
    eng = engine_cls(robot_model, [lo, ma], N, split_env=32, seed=seed)
    eng.step(actions(N, 2), None, *outs(N)); torch.cuda.synchronize()
    got = eng.dr_reset_state.cpu().numpy().T.astype(np.float64)
    for ep, sl in ((lo, slice(0, 32)), (ma, slice(32, 64))):
        exp = R.expected_state(oracle_cls(robot_model, ep), ep, seed, np.arange(sl.start, sl.stop), np.ones(32, np.int64))
        assert (np.abs(got[sl] - exp) / np.maximum(1.0, np.abs(exp))).max() < 2e-5
    eng.close()


def oracle_step(o, phys, task, cnt, drc, act, gr, seed):
    return o.step_dr(phys, task, cnt, drc, act.astype(np.float64), clip_actions=1.0, goal_rand=gr, seed=seed)[:3]


@pytest.mark.parametrize("block", ["loco", "mani", "loco_cc"])
def test_dynamics_from_the_drawn_state(robot_model, engine_cls, oracle_cls, block):
    """The step that resets, and 11 more, against the oracle started from the expected drawn state: Oracle.reset on the flagged envs, their phys
    columns overwritten with the draws, then a step without the flag.  Only the four reset channels are on, so no other on_reset key or noise
    counter enters.  Thresholds and exclusion rule of test_domain_randomisation_step_parity (an env-step whose observations differ by more than
    5e-3 is left out of the other comparisons; at most 2 % of env-steps may be).  tools/reset_dr_oracle_check.py is the CPU pre-check of the
    reference side on these seeds (float32 against float64 oracle, run freely: none left out)."""
    make = DRAW_BLOCKS[block]
    N, seed = R.DYN_ENVS, R.DYN_SEED
    # ---- the construction is sound: at nominal draws, Oracle.reset + a step without the flag is a step with the flag
    ep0 = make(dr_enabled=1, dr_min_frequency=0)
    o0 = oracle_cls(robot_model, ep0); rng0 = np.random.default_rng(3)
    a0, g0 = R.dyn_actions(rng0, N), R.dyn_goal_rand(rng0, N)
    s1, s2 = o0.new_state(N), o0.new_state(N)
    r1 = oracle_step(o0, *s1, o0.new_dr_counters(N), a0, g0, seed)
    assert len(R.oracle_reset_with_draws(o0, ep0, *s2, g0, seed, channels=[DRChannel()] * 4)) == N and not s2[2][:, 3].any()
    r2 = oracle_step(o0, *s2, o0.new_dr_counters(N), a0, g0, seed)
    assert all(np.array_equal(x, y) for x, y in zip(r1, r2)) and all(np.array_equal(x, y) for x, y in zip(s1, s2))
    # ---- the GPU against the oracle from the drawn state
    ep = randomised(make)
    o = oracle_cls(robot_model, ep); eng = engine_cls(robot_model, [ep], N, seed=seed); eng.obs_buf
    rng = np.random.default_rng(R.DYN_ACTION_SEED)
    phys, task, cnt = o.new_state(N); drc = o.new_dr_counters(N)
    bad_total, resets_seen = 0, 0
    for t in range(R.DYN_STEPS + 1):
        # both sides start every step from the oracle's state
        eng.set_phys_env_major(phys); eng.set_task_env_major(task); eng.set_cnt_env_major(cnt)
        act, gr = R.dyn_actions(rng, N), R.dyn_goal_rand(rng, N)
        rows = R.oracle_reset_with_draws(o, ep, phys, task, cnt, gr, seed); resets_seen += len(rows)
        drawn = phys.copy()
        obs, states, rew = oracle_step(o, phys, task, cnt, drc, act, gr, seed)
        out = outs(N, ep.num_obs); eng.step(torch.as_tensor(act, device="cuda"), torch.as_tensor(gr, device="cuda"), *out); torch.cuda.synchronize()
        gobs, gst, grew, grs, gex = [x.cpu().numpy() for x in out]
        if len(rows):          # the engine started these envs from the same drawn state
            rs = eng.dr_reset_state.cpu().numpy().T[rows]; fb = 0 if block != "mani" else 37
            ref = np.concatenate([drawn[rows, 13:37], drawn[rows, fb:fb + 7]], axis=1)
            assert (np.abs(rs - ref) / np.maximum(1.0, np.abs(ref))).max() < 2e-5
        d = np.abs(gobs - np.clip(obs, -5, 5)).max(1)
        bad = d > 5e-3; bad_total += int(bad.sum()); ok = ~bad
        print(f"{block} step {t}: resets {len(rows)}, left out {int(bad.sum())}, median obs diff {np.median(d):.2e}, max {d.max():.2e}")
        assert np.median(d) < 3e-4
        assert np.abs(gst[ok] - np.clip(states[ok], -5, 5)).max() < 5e-3
        assert np.abs(grew[ok] - rew[ok]).max() < 5e-3 * max(1.0, np.abs(rew).max())
        assert np.abs(eng.obs_buf.cpu().numpy()[ok] - obs[ok]).max() < 5e-3
        assert (grs[ok] != cnt[ok, 3]).mean() < 0.01
        c2 = eng.get_cnt_env_major()
        assert np.array_equal(c2[:, 4], cnt[:, 4]) and np.array_equal(c2[:, 5], cnt[:, 5])
        assert np.abs(eng.get_task_env_major()[:, 36:40] - task[:, 36:40]).max() < 1e-6          # same goals
    assert bad_total <= 0.02 * (R.DYN_STEPS + 1) * N, bad_total
    assert resets_seen >= N
    eng.close()


def force_resets(eng, idx):
    eng.cnt[3, torch.as_tensor(idx, device="cuda")] = 1


def test_gate_closed_is_bit_identical_to_an_engine_without_the_channels(robot_model, engine_cls):
    """min_frequency larger than the run: every reset gives the nominal state, and state, outputs and counters are bit-identical to an engine
    with dr_enabled = 1 and no reset channel, over 20 steps with forced resets."""
    N = 256
    for make in (loco_params, mani_cc_params):
        ep = randomised(make, min_frequency=1000)
        e1 = engine_cls(robot_model, [ep], N, seed=11); e2 = engine_cls(robot_model, [dataclasses.replace(ep, dr_reset=[DRChannel() for _ in range(4)])], N, seed=11)
        nominal = torch.as_tensor(R.nominal_state(ep), dtype=torch.float32, device="cuda")
        for t in range(20):
            a = actions(N, 100 + t); o1, o2 = outs(N, ep.num_obs), outs(N, ep.num_obs)
            for e in (e1, e2):
                force_resets(e, np.arange(t % 7, N, 7))
            e1.step(a, None, *o1); e2.step(a, None, *o2); torch.cuda.synchronize()
            assert all(torch.equal(x, y) for x, y in zip(o1, o2))
            assert torch.equal(e1.state, e2.state) and torch.equal(e1.cnt, e2.cnt) and torch.equal(e1.dr_cnt, e2.dr_cnt) and torch.equal(e1.dr_phys, e2.dr_phys)
            assert torch.equal(e1.dr_reset_state, nominal[:, None].expand(31, N))
        assert (e1.cnt[5] >= 3).all()
        e1.close(); e2.close()


def test_gate_follows_min_frequency(robot_model, engine_cls, oracle_cls):
    """min_frequency 3: an env reset before 3 steps have passed since the last randomisation gets the nominal state, one reset after gets a draw."""
    N, seed = 64, 19
    ep = randomised(loco_params, min_frequency=3, max_episode=1000)
    eng = engine_cls(robot_model, [ep], N, seed=seed)
    nominal = R.nominal_state(ep)
    early, late = np.arange(0, 16), np.arange(16, 32)
    zero = torch.zeros(N, 12, device="cuda")
    for t in range(5):
        if t == 2: force_resets(eng, early)
        if t == 4: force_resets(eng, late)
        before = eng.cnt[5].cpu().numpy().copy()
        eng.step(zero, None, *outs(N)); torch.cuda.synchronize()
        rs = eng.dr_reset_state.cpu().numpy().T.astype(np.float64)
        if t == 0:          # the initial reset of every env: the counter stands at 0 < 3
            assert np.array_equal(rs.astype(np.float32), np.tile(nominal.astype(np.float32), (N, 1)))
        if t == 2:
            assert np.array_equal(rs[early].astype(np.float32), np.tile(nominal.astype(np.float32), (16, 1)))
        if t == 4:
            exp = R.expected_state(oracle_cls(robot_model, ep), ep, seed, late, before[late] + 1)
            assert (np.abs(rs[late] - exp) / np.maximum(1.0, np.abs(exp))).max() < 2e-5 and np.abs(rs[late] - nominal).max() > 0.05
            assert np.array_equal(rs[early].astype(np.float32), np.tile(nominal.astype(np.float32), (16, 1)))          # the record stays until the next reset
    dc = eng.dr_cnt.cpu().numpy()
    assert (dc[4][late] == before[late] + 1).all() and (dc[4][early] == 0).all() and (dc[3][late] == 1).all()
    eng.close()


def run(eng, steps, N, num_obs, every=5, record=None):
    for t in range(steps):
        if t % every == every - 1:
            force_resets(eng, np.arange((t // every) % 3, N, 3))
        eng.step(actions(N, 500 + t), None, *outs(N, num_obs))
        if record is not None:
            record.append((eng.cnt[5].clone(), eng.dr_reset_state.clone()))
    torch.cuda.synchronize()


def test_determinism_keys_and_checkpoint(robot_model, engine_cls):
    N = 128
    ep = randomised(loco_params)
    e1, e2, e3 = (engine_cls(robot_model, [ep], N, seed=s) for s in (7, 7, 8))
    rec1, rec3 = [], []
    run(e1, 30, N, 64, record=rec1); run(e2, 30, N, 64); run(e3, 30, N, 64, record=rec3)
    assert torch.equal(e1.state, e2.state) and torch.equal(e1.cnt, e2.cnt) and torch.equal(e1.dr_reset_state, e2.dr_reset_state)
    assert not torch.equal(rec1[0][1], rec3[0][1]) and (rec1[0][1] - rec3[0][1]).abs().max() > 0.05          # another seed, other draws
    first = rec1[0][1]                                                       # episode 1 of every env
    assert (first[:, 0] - first[:, 1]).abs().max() > 0.01                    # two envs, same episode
    assert torch.unique(first[0]).numel() >= N - 2
    later = next(r for ep_no, r in rec1 if (ep_no[0] >= 2))                   # env 0 in a later episode
    assert (later[:, 0] - first[:, 0]).abs().max() > 0.01
    # checkpoint: a new engine continues with identical draws (they are stateless: keyed by seed, env and episode number)
    sd = e1.state_dict()
    e4 = engine_cls(robot_model, [ep], N, seed=1234); e4.load_state_dict(sd)
    run(e1, 12, N, 64); run(e4, 12, N, 64)
    assert torch.equal(e1.state, e4.state) and torch.equal(e1.cnt, e4.cnt) and torch.equal(e1.dr_cnt, e4.dr_cnt)
    assert (e1.cnt[5] > sd["cnt"][5].to("cuda")).any() and torch.equal(e1.dr_reset_state[:, e1.cnt[5] > sd["cnt"][5].to("cuda")], e4.dr_reset_state[:, e4.cnt[5] > sd["cnt"][5].to("cuda")])
    for e in (e1, e2, e3, e4): e.close()


def test_survives_the_reference_amplitudes(robot_model, engine_cls):
    """4096 locomotion envs at the reference's amplitudes, min_frequency 0, 200 random-action steps: no contained blow-up, every state finite."""
    N = 4096
    eng = engine_cls(robot_model, [randomised(loco_params)], N, seed=3)
    o = outs(N)
    for t in range(200):
        eng.step(actions(N, 1000 + t), None, *o)
    torch.cuda.synchronize()
    resets = int(eng.cnt[5].sum().item())
    print(f"blow-ups {eng.blowups} over {resets} randomised resets")
    assert eng.blowups == 0 and torch.isfinite(eng.state).all() and torch.isfinite(o[0]).all() and resets >= N
    eng.close()


def test_through_the_public_interface():
    """A user's YAML reaches the kernel: make_env with the four entries at the reference's values and min_frequency 0."""
    import math
    import warnings
    import locomanipulationrl_amd as lm
    e = lambda prm: {"on_reset": dict(operation="additive", distribution="uniform", distribution_parameters=prm)}
    rp = {"articulation_views": {"robot_view": {"joint_positions": e([-0.1, 0.1]), "joint_velocities": e([-0.1, 0.1]),
                                                "position": e([[-0.05, -0.05, 0.0], [0.05, 0.05, 0.1]]), "orientation": e([[-0.1, -0.1, -1.2], [0.1, 0.1, 1.2]])}}}
    N = 4096
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = lm.make_env("QuadrupedPoseControlCustomController", num_envs=N,
                          overrides={"task": {"domain_randomization": {"randomize": True, "min_frequency": 0, "randomization_params": rp}}})
    env.reset()
    env.step(torch.zeros(N, 12, device="cuda")); torch.cuda.synchronize()
    ep = env._task.engine_params()[0]
    assert ep.dr_min_frequency == 0 and all(ch.enabled for ch in ep.dr_reset)
    rs = env._task.engine.dr_reset_state.cpu().numpy().astype(np.float64)
    dq = rs[0:12] - np.asarray(ep.init_q)[:, None]
    assert abs(dq.std() / (0.2 / math.sqrt(12)) - 1) < 0.10 and np.abs(dq).max() <= 0.1 + 1e-5
    dz = rs[26] - ep.init_base_pos[2]
    assert dz.min() >= -1e-6 and dz.max() <= 0.1 + 1e-6 and dz.std() > 0.02
    w, x, y, z = rs[27:31]
    yaw = np.arctan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))
    assert yaw.min() < -1.0 and yaw.max() > 1.0 and np.abs(yaw).max() <= 1.2 + 1e-3
    assert np.abs(rs[12:24]).max() <= 0.1 + 1e-6 and rs[12:24].std() > 0.04
    env.close()


def test_entry_point_refusals(robot_model, engine_cls):
    """lm_set_reset_randomization needs a live handle, so its refusals are checked here (LM_EINVAL = -1, with a message)."""
    from locomanipulationrl_amd import lib as lmlib
    plain = engine_cls(robot_model, [loco_params()], 64)
    ok = lmlib.make_reset_dr(randomised(loco_params))
    assert plain.lib.lm_set_reset_randomization(plain._h, 0, C.byref(ok)) == -1 and b"dr_enabled" in plain.lib.lm_last_error()
    with pytest.raises(lmlib.EngineError):
        plain.dr_reset_state
    with pytest.raises(lmlib.EngineError):
        engine_cls(robot_model, [loco_params(dr_reset=R.reference_channels())], 64)          # channels on an engine without dr_enabled
    plain.close()
    eng = engine_cls(robot_model, [loco_params(dr_enabled=1)], 64)
    call = lambda rd, block=0: eng.lib.lm_set_reset_randomization(eng._h, block, C.byref(rd))
    assert call(ok) == 0 and call(ok, 1) == -1 and call(ok, -1) == -1
    assert eng.lib.lm_set_reset_randomization(eng._h, 0, None) == -1

    def bad(c, **kw):
        rd = lmlib.make_reset_dr(randomised(loco_params))
        for k, v in kw.items():
            if k in ("p0", "p1"):
                for i, x in enumerate(v): getattr(rd.ch[c], k)[i] = x
            else:
                setattr(rd.ch[c], k, v)
        return rd
    assert call(bad(DR_RESET_JOINT_POS, operation=3)) == -1 and call(bad(DR_RESET_POSITION, distribution=-1)) == -1
    assert call(bad(DR_RESET_JOINT_POS, interval=2)) == -1 and b"on_reset" in eng.lib.lm_last_error()
    assert call(bad(DR_RESET_ORIENTATION, interval=-1)) == -1
    assert call(bad(DR_RESET_JOINT_VEL, operation=1)) == -1 and b"scaling" in eng.lib.lm_last_error()
    assert call(bad(DR_RESET_ORIENTATION, operation=1)) == -1 and b"scaling" in eng.lib.lm_last_error()
    assert call(bad(DR_RESET_JOINT_POS, distribution=2)) == -1 and b"log-uniform" in eng.lib.lm_last_error()          # bounds -0.1 / 0.1
    assert call(bad(DR_RESET_POSITION, distribution=2, p0=[0.1, 0.1, 0.0], p1=[0.2, 0.2, 0.2])) == -1
    assert call(bad(DR_RESET_POSITION, p1=[0.05, float("nan"), 0.1])) == -1
    assert call(bad(DR_RESET_JOINT_POS, distribution=2, p0=[0.1, -1.0, -1.0], p1=[0.2, -1.0, -1.0])) == 0          # the joint channels read slot 0 only
    eng.close()
