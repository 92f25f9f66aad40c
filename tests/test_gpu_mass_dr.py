"""Mass randomisation on the MI355X: k_step_dr / k_step_dr_pd draw the plate's mass, its density factor and the 21 body masses
per env inside the step launch and record what they used in Engine.dr_mass.  The draws are arithmetic on the oracle's `dr_sample`; the dynamics
are checked against per-env oracles built from the recorded masses (the oracle takes the robot model and the plate parameters per instance)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from locomanipulationrl_amd.engine_config import (DR_DISTRIBUTIONS, DR_MASS_BODIES, DR_MASS_FLOOR, DR_MASS_PLATE, DR_MASS_PLATE_DENSITY, DR_ON_STARTUP,
                                                  DR_OPERATIONS, DR_STREAM_MASS, DRChannel, loco_cc_params, loco_params, mani_params)

pytestmark = pytest.mark.gpu

MAKE = {"loco": loco_params, "mani": mani_params, "loco_cc": loco_cc_params}
F32 = np.float32


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


def chan(op, dist, lo, hi, interval):
    return DRChannel(enabled=1, operation=DR_OPERATIONS[op], distribution=DR_DISTRIBUTIONS[dist], interval=interval, p0=[float(lo)] * 3, p1=[float(hi)] * 3)


def with_mass(make, plate=None, density=None, bodies=None, body_p0=None, body_p1=None, **kw):
    """A randomised block with the given mass channels; the body channel's parameters per body (table order) default to its scalar pair."""
    dm = [DRChannel(), DRChannel(), DRChannel()]
    if plate is not None: dm[DR_MASS_PLATE] = plate
    if density is not None: dm[DR_MASS_PLATE_DENSITY] = density
    if bodies is not None:
        dm[DR_MASS_BODIES] = bodies
        body_p0 = [bodies.p0[0]] * 21 if body_p0 is None else [float(x) for x in body_p0]
        body_p1 = [bodies.p1[0]] * 21 if body_p1 is None else [float(x) for x in body_p1]
        kw.update(dr_mass_body_p0=body_p0, dr_mass_body_p1=body_p1)
    return make(dr_enabled=1, dr_mass=dm, **kw)


def table_masses(rm):
    """Nominal body masses in table order, as the engine holds them (float32)."""
    return np.asarray([rm.mass[k] for k in rm.table_body_order()], dtype=np.float32)


def apply(op, nominal, n):
    return nominal + n if op == DR_OPERATIONS["additive"] else nominal * n if op == DR_OPERATIONS["scaling"] else n


def expected_record(ora, rm, ep, seed, N, dr_step, reset_key, env0=0):
    """[23][N]: operation(nominal, dr_sample(seed, stream, env, key, component, ...)) floored at 0.05 x nominal; rows of channels that are off are nominal."""
    exp = np.zeros((23, N)); nom_b = table_masses(rm).astype(np.float64)
    key = lambda ch: dr_step // ch.interval if ch.interval > 0 else (0 if ch.interval < 0 else reset_key)
    cp, cd, cb = ep.dr_mass[DR_MASS_PLATE], ep.dr_mass[DR_MASS_PLATE_DENSITY], ep.dr_mass[DR_MASS_BODIES]
    for e in range(N):
        s = 1.0
        if cd.enabled:
            s = max(apply(cd.operation, 1.0, ora.dr_sample(seed, DR_STREAM_MASS + DR_MASS_PLATE_DENSITY, env0 + e, key(cd), 0, cd.distribution, cd.p0[0], cd.p1[0])), DR_MASS_FLOOR)
        nom = s * float(F32(ep.plate_mass)); m = nom
        if cp.enabled:
            m = max(apply(cp.operation, nom, ora.dr_sample(seed, DR_STREAM_MASS + DR_MASS_PLATE, env0 + e, key(cp), 0, cp.distribution, cp.p0[0], cp.p1[0])), DR_MASS_FLOOR * nom)
        exp[0, e], exp[1, e] = m, s
        for c in range(21):
            mb = nom_b[c]
            if cb.enabled:
                n = ora.dr_sample(seed, DR_STREAM_MASS + DR_MASS_BODIES, env0 + e, key(cb), c, cb.distribution, ep.dr_mass_body_p0[c], ep.dr_mass_body_p1[c])
                mb = max(apply(cb.operation, nom_b[c], n), DR_MASS_FLOOR * nom_b[c])
            exp[2 + c, e] = mb
    return exp


def draw_cases(rm):
    m = table_masses(rm).astype(np.float64)
    return {
        # every operation x distribution once, all three triggers, scalar and per-body parameters
        "loco-scaling-uniform-startup": ("loco", dict(bodies=chan("scaling", "uniform", 0.5, 2.0, DR_ON_STARTUP))),
        "loco_cc-scaling-loguniform-reset": ("loco_cc", dict(bodies=chan("scaling", "loguniform", 0.5, 2.0, 0))),
        "loco-additive-gaussian-interval-per-body": ("loco", dict(bodies=chan("additive", "gaussian", 0.0, 0.0, 2), body_p0=np.zeros(21), body_p1=0.2 * m)),
        "loco_cc-additive-loguniform-startup": ("loco_cc", dict(bodies=chan("additive", "loguniform", 0.01, 0.1, DR_ON_STARTUP))),
        "mani-direct-uniform-per-body+scaling-gaussian-plate": ("mani", dict(bodies=chan("direct", "uniform", 0.0, 0.0, DR_ON_STARTUP), body_p0=0.5 * m, body_p1=2.0 * m,
                                                                           plate=chan("scaling", "gaussian", 1.0, 0.2, 3))),
        "mani-additive-uniform-plate-reset": ("mani", dict(plate=chan("additive", "uniform", -1.0, 1.0, 0))),
        "mani-direct-gaussian-plate+density": ("mani", dict(plate=chan("direct", "gaussian", 2.0, 0.3, DR_ON_STARTUP), density=chan("scaling", "uniform", 0.5, 2.0, DR_ON_STARTUP))),
        "mani-direct-loguniform-plate-reset+density": ("mani", dict(plate=chan("direct", "loguniform", 1.0, 4.0, 0), density=chan("scaling", "loguniform", 0.5, 2.0, DR_ON_STARTUP))),
        "mani-scaling-plate-on-density": ("mani", dict(plate=chan("scaling", "uniform", 0.5, 2.0, 1), density=chan("scaling", "gaussian", 1.0, 0.1, DR_ON_STARTUP))),
    }


CASE_NAMES = ["loco-scaling-uniform-startup", "loco_cc-scaling-loguniform-reset", "loco-additive-gaussian-interval-per-body", "loco_cc-additive-loguniform-startup",
              "mani-direct-uniform-per-body+scaling-gaussian-plate", "mani-additive-uniform-plate-reset", "mani-direct-gaussian-plate+density",
              "mani-direct-loguniform-plate-reset+density", "mani-scaling-plate-on-density"]


@pytest.mark.parametrize("case", CASE_NAMES)
def test_draws_match_the_oracle_samples(robot_model, engine_cls, oracle_cls, case):
    """64 envs, min_frequency 0, every env flagged, dr_step 5: after one step Engine.dr_mass is operation(nominal, dr_sample(...)) floored, within
    2e-5 per unit of magnitude (float32 against the float64 oracle: the log / cos inside dr_sample)."""
    cases = draw_cases(robot_model)
    assert sorted(cases) == sorted(CASE_NAMES)
    block, kw = cases[case]
    N, seed = 64, 23
    ep = with_mass(MAKE[block], dr_min_frequency=0, **kw)
    eng = engine_cls(robot_model, [ep], N, seed=seed)
    nominal = np.concatenate([[F32(ep.plate_mass), F32(1.0)], table_masses(robot_model)])
    assert np.array_equal(eng.dr_mass.cpu().numpy(), np.tile(nominal[:, None], (1, N)))          # before the first step: the nominal values
    assert eng.dr_plate_mass.shape == (N,) and eng.dr_body_masses.shape == (21, N)
    eng.dr_cnt[2].fill_(5)
    eng.step(torch.zeros(N, 12, device="cuda"), None, *outs(N, ep.num_obs)); torch.cuda.synchronize()
    got = eng.dr_mass.cpu().numpy().astype(np.float64)
    exp = expected_record(oracle_cls(robot_model, ep), robot_model, ep, seed, N, 5, 1)
    assert (np.abs(got - exp) / np.maximum(1.0, np.abs(exp))).max() < 2e-5, case
    on = [r for r in range(23) if (r == 0 and (ep.dr_mass[0].enabled or ep.dr_mass[1].enabled)) or (r == 1 and ep.dr_mass[1].enabled) or (r >= 2 and ep.dr_mass[2].enabled)]
    for r in on:
        assert len(np.unique(got[r])) > N // 2, (case, r)          # drawn per env ...
    for r in set(range(23)) - set(on):
        assert (got[r] == nominal[r]).all(), (case, r)            # ... and only where a channel is on
    if ep.dr_mass[2].enabled:
        assert np.abs(np.corrcoef(got[2], got[3])[0, 1]) < 0.5    # one draw per body, not one per env
    assert (got > 0).all() and torch.isfinite(eng.state).all()
    eng.close()


def test_a_gaussian_tail_is_floored(robot_model, engine_cls, oracle_cls):
    """additive N(-m, 0.1 m) puts the mass around zero: every draw below 0.05 m is recorded (and used) as 0.05 m."""
    N, seed = 64, 5
    m = table_masses(robot_model).astype(np.float64)
    ep = with_mass(loco_params, bodies=chan("additive", "gaussian", 0.0, 0.0, 1), body_p0=-m, body_p1=0.1 * m)
    eng = engine_cls(robot_model, [ep], N, seed=seed)
    o = outs(N); eng.step(torch.zeros(N, 12, device="cuda"), None, *o); torch.cuda.synchronize()
    got = eng.dr_body_masses.cpu().numpy()
    ora = oracle_cls(robot_model, ep)
    raw = np.array([[m[c] + ora.dr_sample(seed, DR_STREAM_MASS + DR_MASS_BODIES, e, 0, c, DR_DISTRIBUTIONS["gaussian"], -m[c], 0.1 * m[c]) for e in range(N)] for c in range(21)])
    floor64 = DR_MASS_FLOOR * m[:, None]
    exp = np.maximum(raw, floor64)
    hit = raw < floor64
    assert 0.5 * hit.size < hit.sum() < hit.size          # ~ 69 % of N(0, 0.1 m) lies below 0.05 m
    floor = np.broadcast_to((F32(DR_MASS_FLOOR) * m.astype(F32))[:, None], got.shape)
    clear = np.abs(raw - floor64) > 1e-5          # away from the threshold, where float32 and float64 agree on the side
    assert np.array_equal(got[hit & clear], floor[hit & clear]) and (got[~hit & clear] > floor[~hit & clear]).all()
    assert (np.abs(got - exp) / np.maximum(1.0, np.abs(exp))).max() < 2e-5 and (got >= floor).all()
    assert torch.isfinite(o[0]).all()
    eng.close()


# ---- step parity against per-env oracles
def parity_cases():
    return {
        "loco-bodies": ("loco", dict(bodies=chan("scaling", "uniform", 0.5, 2.0, DR_ON_STARTUP)), True),
        "loco_cc-bodies": ("loco_cc", dict(bodies=chan("scaling", "uniform", 0.5, 2.0, DR_ON_STARTUP)), True),
        "mani-plate-mass": ("mani", dict(plate=chan("scaling", "uniform", 0.5, 2.0, 2)), True),
        "mani-plate-density": ("mani", dict(density=chan("scaling", "uniform", 0.5, 2.0, DR_ON_STARTUP)), False),
    }


@pytest.mark.parametrize("case", list(parity_cases()))
def test_step_parity_against_per_env_oracles(robot_model, engine_cls, oracle_cls, case):
    """40 envs (two full wavefronts and a half-empty one), 8 random-action steps, both sides restarted from the oracle's state every step.  Each
    env is compared with an oracle built from ITS recorded masses: median of the per-env max observation error < 3e-4 per step, rewards within
    5e-3 relative on the kept envs, at most 2 % of the env-steps beyond 5e-3.  Negative control (mass / body_masses cases): against the
    nominal-mass oracle from the same states the per-step median exceeds 3e-3, ten times the pass threshold, in steps 1 to 7."""
    block, kw, control = parity_cases()[case]
    make = MAKE[block]
    N, seed, steps = 40, 17, 8
    ep = with_mass(make, **kw)
    eng = engine_cls(robot_model, [ep], N, seed=seed); eng.obs_buf
    o0 = oracle_cls(robot_model, make())
    order = robot_model.table_body_order()
    phys, task, cnt = o0.new_state(N)
    rng = np.random.default_rng(3)
    oracles = {}
    bad_total = 0; control_medians = []

    def oracle_of(rec):
        k = rec.tobytes()
        if k not in oracles:
            mass = np.array(robot_model.mass, dtype=np.float64)
            for s, b in enumerate(order):
                mass[b] = float(rec[2 + s])
            p = make(plate_mass=float(rec[0]), plate_inertia=[float(rec[1]) * x for x in make().plate_inertia])
            oracles[k] = oracle_cls(dataclasses.replace(robot_model, mass=mass), p)
        return oracles[k]
    for t in range(steps):
        eng.set_phys_env_major(phys); eng.set_task_env_major(task); eng.set_cnt_env_major(cnt)
        eng.dr_cnt[2].fill_(t)          # the on_interval key runs on the per-env dr_step counter
        act = rng.uniform(-1.0, 1.0, size=(N, 12)).astype(np.float32)
        out = outs(N, ep.num_obs); eng.step(torch.as_tensor(act, device="cuda"), None, *out); torch.cuda.synchronize()
        gobs, gst, grew, grs, gex = [x.cpu().numpy() for x in out]
        rec = eng.dr_mass.cpu().numpy()
        goal = np.stack([o0.hash_uniform3(seed, e, int(cnt[e, 5])) for e in range(N)])
        if control:
            p, tk, c = phys.copy(), task.copy(), cnt.copy()
            obs0, _, _, _ = o0.step(p, tk, c, act.astype(np.float64), goal_rand=goal, seed=seed)
            control_medians.append(float(np.median(np.abs(gobs - np.clip(obs0, -5, 5)).max(1))))
        obs = np.zeros((N, ep.num_obs)); rew = np.zeros(N)
        for e in range(N):
            p, tk, c = phys[e:e + 1].copy(), task[e:e + 1].copy(), cnt[e:e + 1].copy()
            ob, _, rw, _ = oracle_of(rec[:, e]).step(p, tk, c, act[e:e + 1].astype(np.float64), goal_rand=goal[e:e + 1], seed=seed)
            phys[e], task[e], cnt[e] = p[0], tk[0], c[0]
            obs[e], rew[e] = ob[0], rw[0]
        d = np.abs(gobs - np.clip(obs, -5, 5)).max(1)
        bad = d > 5e-3; bad_total += int(bad.sum()); ok = ~bad
        print(f"{case} step {t}: median {np.median(d):.3e} max {d.max():.3e} left out {int(bad.sum())}" + (f" control median {control_medians[-1]:.3e}" if control else ""))
        assert np.median(d) < 3e-4, (t, np.median(d))
        assert np.abs(grew[ok] - rew[ok]).max() < 5e-3 * max(1.0, np.abs(rew).max()), t
    assert bad_total <= 0.02 * steps * N, bad_total
    rec = eng.dr_mass.cpu().numpy()
    assert len(oracles) >= N and len(np.unique(rec[1 if "density" in case else 0 if block == "mani" else 2])) == N          # the envs really differ
    if control:
        assert min(control_medians[1:]) > 3e-3, control_medians
    eng.close()


@pytest.mark.parametrize("block", ["loco", "loco_cc", "mani"])
def test_nominal_draw_is_a_noop_bit_for_bit(robot_model, engine_cls, block):
    """body_masses scaling uniform [1, 1] redrawn every step against a randomised engine without mass channels: every output, the state, the
    counters and the sampled attributes are bit-identical over 6 random-action steps (the hub's update is written so that m' = m is exact)."""
    N = 128; make = MAKE[block]
    e1 = engine_cls(robot_model, [with_mass(make, bodies=chan("scaling", "uniform", 1.0, 1.0, 1))], N, seed=9)
    e2 = engine_cls(robot_model, [make(dr_enabled=1)], N, seed=9)
    nobs = e1.num_obs
    g = torch.Generator(device="cuda").manual_seed(5)
    for t in range(6):
        a = torch.rand(N, 12, device="cuda", generator=g) * 2.4 - 1.2
        o1, o2 = outs(N, nobs), outs(N, nobs)
        e1.step(a, None, *o1); e2.step(a, None, *o2)
        torch.cuda.synchronize()
        for x, y in zip(o1, o2):
            assert torch.equal(x, y), t
    assert torch.equal(e1.state, e2.state) and torch.equal(e1.cnt, e2.cnt) and torch.equal(e1.dr_phys, e2.dr_phys) and torch.equal(e1.dr_mu, e2.dr_mu)
    assert torch.equal(e1.dr_mass, e2.dr_mass)          # the drawn masses ARE the nominal ones
    e1.close(); e2.close()


def test_density_is_mass_and_inertia_together_bit_for_bit(robot_model, engine_cls):
    """density x 1.5 on the nominal plate against density x 1 on a plate whose mass and inertia were multiplied by 1.5 (in float32, as the kernel
    multiplies): the same plate, so bit-identical outputs over 6 steps."""
    N = 128
    base = mani_params()
    f = lambda x: float(F32(1.5) * F32(x))
    eA = engine_cls(robot_model, [with_mass(mani_params, density=chan("scaling", "uniform", 1.5, 1.5, DR_ON_STARTUP))], N, seed=9)
    eB = engine_cls(robot_model, [with_mass(mani_params, density=chan("scaling", "uniform", 1.0, 1.0, DR_ON_STARTUP), plate_mass=f(base.plate_mass),
                                            plate_inertia=[f(x) for x in base.plate_inertia])], N, seed=9)
    g = torch.Generator(device="cuda").manual_seed(5)
    for t in range(6):
        a = torch.rand(N, 12, device="cuda", generator=g) * 2.4 - 1.2
        o1, o2 = outs(N), outs(N)
        eA.step(a, None, *o1); eB.step(a, None, *o2)
        torch.cuda.synchronize()
        for x, y in zip(o1, o2):
            assert torch.equal(x, y), t
    assert torch.equal(eA.state, eB.state) and torch.equal(eA.cnt, eB.cnt)
    assert torch.equal(eA.dr_plate_mass, eB.dr_plate_mass) and (eA.dr_mass[1] == 1.5).all() and (eB.dr_mass[1] == 1.0).all()
    assert abs(float(eA.dr_plate_mass[0]) - 3.6) < 1e-6
    # and the factor matters: the nominal plate moves differently
    eC = engine_cls(robot_model, [mani_params(dr_enabled=1)], N, seed=9)
    g = torch.Generator(device="cuda").manual_seed(5)
    for t in range(6):
        eC.step(torch.rand(N, 12, device="cuda", generator=g) * 2.4 - 1.2)
    assert (eC.state[:50] - eA.state[:50]).abs().max() > 1e-3
    eA.close(); eB.close(); eC.close()


# ---- triggers (modelled on the friction tests)
def run(eng, steps, N):
    """Random-action steps; per step the counters before it and the mass record after it."""
    g = torch.Generator(device="cuda").manual_seed(1)
    recs, pre = [], []
    for _ in range(steps):
        pre.append((eng.cnt[3].cpu().numpy().copy(), eng.dr_cnt.cpu().numpy().copy()))
        eng.step(torch.rand(N, 12, device="cuda", generator=g) * 2 - 1)
        recs.append(eng.dr_mass.cpu().numpy().copy())
    return np.array(recs), pre


def test_on_startup_is_fixed_per_env(robot_model, engine_cls):
    N = 64
    ch = chan("scaling", "uniform", 0.5, 2.0, DR_ON_STARTUP)
    eng = engine_cls(robot_model, [with_mass(loco_params, bodies=ch, max_episode=4)], N, seed=2)
    recs, pre = run(eng, 14, N)
    assert sum(int(r.sum()) for r, _ in pre[1:]) >= N          # resets happened (4-step episodes)
    assert (recs == recs[0]).all()                              # constant across steps and resets ...
    nom = table_masses(robot_model)[:, None]
    assert all(len(np.unique(recs[0][r])) == N for r in range(2, 23))          # ... different across envs and bodies
    assert (recs[0][2:] >= 0.5 * nom * (1 - 1e-6)).all() and (recs[0][2:] <= 2.0 * nom * (1 + 1e-6)).all()
    eng.reset_all(); eng.step(torch.zeros(N, 12, device="cuda"))
    assert np.array_equal(eng.dr_mass.cpu().numpy(), recs[0])
    # keyed by (seed, stream, env, component) only: a second engine with the same seed draws the same masses, another seed others
    e2 = engine_cls(robot_model, [with_mass(loco_params, bodies=ch)], N, seed=2)
    e2.step(torch.zeros(N, 12, device="cuda"))
    assert np.array_equal(e2.dr_mass.cpu().numpy(), recs[0])
    e3 = engine_cls(robot_model, [with_mass(loco_params, bodies=ch)], N, seed=3)
    e3.step(torch.zeros(N, 12, device="cuda"))
    assert (e3.dr_mass.cpu().numpy()[2:] != recs[0][2:]).mean() > 0.99
    eng.close(); e2.close(); e3.close()


def test_on_reset_follows_the_min_frequency_gate(robot_model, engine_cls):
    N, minf = 64, 3
    ep = with_mass(mani_params, plate=chan("scaling", "uniform", 0.5, 2.0, 0), bodies=chan("scaling", "uniform", 0.8, 1.25, 0), max_episode=2, dr_min_frequency=minf)
    eng = engine_cls(robot_model, [ep], N, seed=4)
    recs, pre = run(eng, 16, N)
    prev = np.tile(np.concatenate([[F32(ep.plate_mass), F32(1.0)], table_masses(robot_model)])[:, None], (1, N))          # before the first gated reset: nominal
    fired = 0
    for t in range(16):
        reset, drc = pre[t]
        gate = (reset != 0) & (drc[3] >= minf)          # a reset that passes min_frequency (randomization_buf >= min_frequency)
        for r in [0] + list(range(2, 23)):
            assert np.array_equal(recs[t][r] != prev[r], gate), (t, r)
        assert (recs[t][1] == 1.0).all()
        fired += int(gate.sum()); prev = recs[t]
    assert fired >= N and (np.array([p[0] for p in pre]) != 0).sum() > fired          # some resets were gated off
    eng.close()


def test_on_interval_follows_frequency_interval(robot_model, engine_cls):
    N, k = 64, 3
    ep = with_mass(mani_params, plate=chan("additive", "gaussian", 0.0, 0.2, k), bodies=chan("scaling", "loguniform", 0.8, 1.25, k), max_episode=5)
    eng = engine_cls(robot_model, [ep], N, seed=6)
    recs, pre = run(eng, 13, N)
    rows = [0] + list(range(2, 23))
    for t in range(1, 13):
        assert (pre[t][1][2] == t).all()
        same = recs[t][rows] == recs[t - 1][rows]
        assert (not same.any()) if t % k == 0 else same.all(), t
    assert len(np.unique(recs[0][0])) == N
    eng.close()


def test_plate_entry_leaves_the_locomotion_half_nominal():
    """Co-training through the task YAML: the plate-mass entry randomises the manipulation half only."""
    import locomanipulationrl_amd as lm
    mp = {"rigid_prim_views": {"plate": {"mass": {"on_interval": dict(frequency_interval=1, operation="scaling", distribution="uniform", distribution_parameters=[0.5, 2.0])}}}}
    env = lm.make_env("JointLocomanipulation", num_envs=128, overrides={"task": {"domain_randomization": {"randomize": True, "randomization_params": mp}}})
    lo, ma = env._task.engine_params()
    assert lo.dr_mass[DR_MASS_PLATE].enabled == 0 and ma.dr_mass[DR_MASS_PLATE].enabled == 1
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(0)
    last = None
    for _ in range(4):
        o, r, d, ex = env.step(torch.rand(128, 12, device="cuda", generator=g) * 2 - 1)
        pm = env._task.engine.dr_plate_mass.cpu().numpy()
        assert (pm[:64] == F32(lo.plate_mass)).all()
        assert len(np.unique(pm[64:])) == 64 and 0.5 * ma.plate_mass - 1e-5 <= pm[64:].min() and pm[64:].max() <= 2.0 * ma.plate_mass + 1e-5
        assert last is None or (pm[64:] != last).all()          # redrawn every step
        last = pm[64:].copy()
    assert (env._task.engine.dr_mass[1] == 1.0).all()
    assert torch.isfinite(o["obs"]).all()
    env.close()


def test_entry_point_refusals(robot_model, engine_cls):
    """lm_set_mass_randomization needs a live handle, so its refusals are checked here (LM_EINVAL = -1, with a message); the engine stays usable."""
    from locomanipulationrl_amd import lib as lmlib
    bodies = chan("scaling", "uniform", 0.5, 2.0, DR_ON_STARTUP)
    plain = engine_cls(robot_model, [loco_params()], 64)
    ok = lmlib.make_mass_dr(with_mass(loco_params, bodies=bodies))
    assert plain.lib.lm_set_mass_randomization(plain._h, 0, C.byref(ok)) == -1 and b"dr_enabled" in plain.lib.lm_last_error()
    with pytest.raises(lmlib.EngineError):
        plain.dr_mass
    with pytest.raises(lmlib.EngineError):
        engine_cls(robot_model, [loco_params(dr_mass=with_mass(loco_params, bodies=bodies).dr_mass, dr_mass_body_p0=[0.5] * 21, dr_mass_body_p1=[2.0] * 21)], 64)
    plain.step(torch.zeros(64, 12, device="cuda")); torch.cuda.synchronize()
    plain.close()

    def refusals(eng, make, cases, good):
        call = lambda md, block=0: eng.lib.lm_set_mass_randomization(eng._h, block, C.byref(md))
        assert call(good) == 0 and call(good, 1) == -1 and call(good, -1) == -1 and b"block" in eng.lib.lm_last_error()
        assert eng.lib.lm_set_mass_randomization(eng._h, 0, None) == -1
        for kw, text in cases:
            assert call(lmlib.make_mass_dr(with_mass(make, **kw))) == -1, kw
            assert text in eng.lib.lm_last_error(), (kw, eng.lib.lm_last_error())
        assert call(good) == 0
        o = outs(64); eng.step(torch.zeros(64, 12, device="cuda"), None, *o); torch.cuda.synchronize()
        assert torch.isfinite(o[0]).all()
    nan = float("nan")
    eng = engine_cls(robot_model, [loco_params(dr_enabled=1)], 64)
    refusals(eng, loco_params, [
        (dict(plate=chan("scaling", "uniform", 0.5, 2.0, 0)), b"manipulation"),                        # plate channels on a locomotion block
        (dict(density=chan("scaling", "uniform", 0.5, 2.0, DR_ON_STARTUP)), b"manipulation"),
        (dict(bodies=chan("scaling", "uniform", 0.0, 2.0, 0)), b"non-positive"),                       # a range reaching <= 0
        (dict(bodies=chan("additive", "uniform", -1.0, 1.0, 0)), b"non-positive"),
        (dict(bodies=chan("direct", "uniform", 0.1, 0.2, 0), body_p0=[0.1] * 20 + [-0.1], body_p1=[0.2] * 21), b"non-positive"),      # the last body's pair
        (dict(bodies=chan("scaling", "loguniform", -0.5, 2.0, 0)), b"log-uniform"),
        (dict(bodies=chan("scaling", "uniform", 0.5, nan, 0)), b"non-finite"),
        (dict(bodies=chan("scaling", "uniform", 0.5, 2.0, -2)), b"interval"),
        (dict(bodies=DRChannel(enabled=1, operation=3, distribution=1, interval=0, p0=[0.5] * 3, p1=[2.0] * 3)), b"operation"),
        (dict(bodies=DRChannel(enabled=1, operation=1, distribution=5, interval=0, p0=[0.5] * 3, p1=[2.0] * 3)), b"distribution"),
    ], ok)
    assert call_ok_gaussian(eng, lmlib)
    eng.close()
    eng = engine_cls(robot_model, [mani_params(dr_enabled=1)], 64)
    good = lmlib.make_mass_dr(with_mass(mani_params, plate=chan("scaling", "uniform", 0.5, 2.0, 2), density=chan("scaling", "uniform", 0.5, 2.0, DR_ON_STARTUP), bodies=bodies))
    refusals(eng, mani_params, [
        (dict(density=chan("scaling", "uniform", 0.5, 2.0, 3)), b"density"),                            # density with an interval
        (dict(density=chan("scaling", "uniform", 0.5, 2.0, 0)), b"density"),
        (dict(density=chan("additive", "uniform", 0.0, 0.1, DR_ON_STARTUP)), b"density"),
        (dict(density=chan("direct", "uniform", 900.0, 1100.0, DR_ON_STARTUP)), b"density"),
        (dict(density=chan("scaling", "uniform", -0.5, 2.0, DR_ON_STARTUP)), b"non-positive"),
        (dict(plate=chan("additive", "uniform", -2.4, 1.0, 0)), b"non-positive"),
        (dict(plate=chan("additive", "uniform", -1.3, 1.0, 0), density=chan("scaling", "uniform", 0.5, 2.0, DR_ON_STARTUP)), b"non-positive"),      # 0.5 x 2.4 - 1.3
        (dict(plate=chan("direct", "loguniform", 0.0, 1.0, 0)), b"log-uniform"),
        (dict(plate=chan("scaling", "gaussian", nan, 1.0, 0)), b"non-finite"),
    ], good)
    eng.close()


def call_ok_gaussian(eng, lmlib):
    """A gaussian whose tail reaches below zero is accepted: the floor takes it."""
    md = lmlib.make_mass_dr(with_mass(loco_params, bodies=chan("additive", "gaussian", -1.0, 1.0, 0)))
    return eng.lib.lm_set_mass_randomization(eng._h, 0, C.byref(md)) == 0
