"""Per-env physics parameters held by the caller, on the MI355X: k_step_dr_hp / k_step_dr_pd_hp replace what the channels drew
by the held rows of the hold table.  Pinned here: held = drawn bit for bit (which carries the per-env-oracle guarantee of the drawing kernels
over to held values), the meaning of held grids against per-env oracles, hold against channel, the refusals, the neighbours (engines that do
not opt in, rollout plans, checkpoints) and an evaluation sweep end to end."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from locomanipulationrl_amd.engine_config import (DR_BASE_FORCE, DR_CHANNELS, DR_DISTRIBUTIONS, DR_GRAVITY, DR_MAT_OTHER, DR_MAT_ROBOT, DR_ON_STARTUP, DR_OPERATIONS,
                                                  DRChannel, loco_cc_params, loco_params, mani_params)

pytestmark = pytest.mark.gpu

MAKE = {"loco": loco_params, "mani": mani_params, "loco_cc": loco_cc_params}
F32 = np.float32
LONG = 1000          # an on_interval period longer than any run here: the key dr_step // LONG never changes


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


def mat(lo, hi):
    """on_startup scaling of the dynamic coefficient (static / restitution neutral)."""
    return DRChannel(enabled=1, operation=DR_OPERATIONS["scaling"], distribution=DR_DISTRIBUTIONS["uniform"], interval=DR_ON_STARTUP, p0=[1.0, lo, 1.0], p1=[1.0, hi, 1.0])


def drawing(block):
    """A block whose channels draw every per-env parameter its family has, with keys that never change: on_startup for material, body masses,
    plate mass + density, gains and latency; on_interval (period LONG) additive / direct for gravity and the base force."""
    make = MAKE[block]
    dr = [DRChannel() for _ in range(DR_CHANNELS)]
    dr[DR_GRAVITY] = DRChannel(enabled=1, operation=DR_OPERATIONS["additive"], distribution=DR_DISTRIBUTIONS["gaussian"], interval=LONG, p0=[0.0, 0.0, 0.0], p1=[0.3, 0.3, 0.5])
    dr[DR_BASE_FORCE] = DRChannel(enabled=1, operation=DR_OPERATIONS["direct"], distribution=DR_DISTRIBUTIONS["uniform"], interval=LONG, p0=[-0.5, -0.5, -0.5], p1=[0.5, 0.5, 0.5])
    dm = [DRChannel(), DRChannel()]; dm[DR_MAT_ROBOT] = mat(0.5, 1.5)
    mass = [DRChannel(), DRChannel(), chan("scaling", "uniform", 0.5, 2.0, DR_ON_STARTUP)]
    act = [DRChannel(), chan("scaling", "loguniform", 0.5, 2.0, DR_ON_STARTUP), DRChannel()]          # kd: every family but effort drive
    if block == "mani":
        dm[DR_MAT_OTHER] = mat(0.6, 1.4)
        mass[0] = chan("scaling", "uniform", 0.5, 2.0, DR_ON_STARTUP); mass[1] = chan("scaling", "uniform", 0.7, 1.5, DR_ON_STARTUP)
    if block == "loco_cc":
        act[0] = chan("scaling", "loguniform", 0.5, 2.0, DR_ON_STARTUP); act[2] = chan("direct", "uniform", 0.0, 6.0, DR_ON_STARTUP)
    return make(dr_enabled=1, dr=dr, dr_mat=dm, dr_mass=mass, dr_mass_body_p0=[0.5] * 21, dr_mass_body_p1=[2.0] * 21, dr_actuator=act)


def records(e):
    return torch.cat([e.dr_phys, e.dr_mu[None]]).clone(), e.dr_mass.clone(), e.dr_actuator.clone()


def hold_records(eng, phys, mass, actuator, blocks):
    """Hold every row the engine's blocks read at the recorded values."""
    named = dict(max_efforts=phys[0:12], max_velocities=phys[12:24], gravity=phys[24:27], base_force=phys[27:30], joint_damping=phys[30:42], mu=phys[42],
                 body_masses=mass[2:], kd=actuator[1])
    if "mani" in blocks:
        named.update(plate_mass=mass[0], plate_inertia_factor=mass[1])
    if "loco_cc" in blocks:
        named.update(kp=actuator[0], latency=actuator[2])
    eng.set_env_params(**named)
    return named


# ---- 1. held = drawn, bit for bit
@pytest.mark.parametrize("case", ["loco", "loco_cc", "mani", "cotrain"])
def test_held_equals_drawn_bit_for_bit(robot_model, engine_cls, case):
    """Engine A draws (keys that never change), engine B has no channel on and holds A's records of the first step: same seed, same random actions,
    6 steps - every output, the state, the counters and the three records are bit-identical.  40 envs = two full wavefronts and a half-empty one;
    32 + 32 for the co-training layout."""
    blocks = ["loco", "mani"] if case == "cotrain" else [case]
    N, split = (64, 32) if case == "cotrain" else (40, None)
    A = engine_cls(robot_model, [drawing(b) for b in blocks], N, split_env=split, seed=17)
    B = engine_cls(robot_model, [MAKE[b](dr_enabled=1) for b in blocks], N, split_env=split, seed=17)
    B.enable_env_params()
    assert A.step_variant == B.step_variant == "w1" and not A.env_params_enabled and B.env_params_enabled and B.env_params_held == []
    nobs = A.num_obs
    g = torch.Generator(device="cuda").manual_seed(5)
    acts = [torch.rand(N, 12, device="cuda", generator=g) * 2.4 - 1.2 for _ in range(6)]
    got_a = []
    for t, a in enumerate(acts):
        o = outs(N, nobs); A.step(a, None, *o); got_a.append(o)
        if t == 0:
            torch.cuda.synchronize()
            rec = records(A)
    torch.cuda.synchronize()
    named = hold_records(B, *rec, blocks)
    assert sorted(B.env_params_held) == sorted(named)
    for k, v in named.items():
        assert torch.equal(B.env_params[k], v), k          # the zero-copy views show what is held
    # the draws really differ per env (else the comparison below says little)
    assert len(torch.unique(rec[0][42])) > N // 2 and len(torch.unique(rec[1][5])) > N // 2 and len(torch.unique(rec[2][1])) > N // 2
    for t, a in enumerate(acts):
        o = outs(N, nobs); B.step(a, None, *o); torch.cuda.synchronize()
        for x, y in zip(got_a[t], o):
            assert torch.equal(x, y), (case, t)
    assert torch.equal(A.state, B.state) and torch.equal(A.cnt, B.cnt) and torch.equal(A.dr_cnt, B.dr_cnt)
    for x, y in zip(records(A), records(B)):
        assert torch.equal(x, y), case
    for x, y in zip(records(A), rec):
        assert torch.equal(x, y), case          # (A's keys never changed)
    A.close(); B.close()


# ---- 2. meaning, against per-env oracles, on grids
def grid_cases(rm):
    m = np.asarray([rm.mass[k] for k in rm.table_body_order()], dtype=np.float32)
    geo = np.geomspace(0.5, 2.0, 40)
    cc = loco_cc_params()
    return {
        "mu": ("loco", dict(mu=np.linspace(0.2, 1.2, 40).astype(F32))),
        "body_masses": ("loco", dict(body_masses=(m[:, None] * geo[None, :]).astype(F32))),
        "kp_kd": ("loco_cc", dict(kp=(cc.pd_kp * geo).astype(F32), kd=(cc.kd * geo[::-1]).astype(F32))),
        "plate_mass": ("mani", dict(plate_mass=(mani_params().plate_mass * geo).astype(F32))),
    }


@pytest.mark.parametrize("case", ["mu", "body_masses", "kp_kd", "plate_mass"])
def test_held_grids_against_per_env_oracles(robot_model, engine_cls, oracle_cls, case):
    """40 envs, 8 random-action steps (seed 17, action rng 3), both sides restarted from the oracle's state every step, as
    test_gpu_mass_dr.py::test_step_parity_against_per_env_oracles does, with that file's thresholds: per-step median of the per-env max
    observation error < 3e-4, rewards within 5e-3 relative on the kept envs, at most 2 % of the env-steps beyond 5e-3; negative control:
    against the nominal oracle the per-step median exceeds 3e-3 in every step."""
    block, held = grid_cases(robot_model)[case]
    make = MAKE[block]
    N, seed, steps = 40, 17, 8
    ep = make(dr_enabled=1)
    eng = engine_cls(robot_model, [ep], N, seed=seed); eng.obs_buf
    eng.enable_env_params(); eng.set_env_params(**held)
    o0 = oracle_cls(robot_model, make())
    order = robot_model.table_body_order()
    phys, task, cnt = o0.new_state(N)
    rng = np.random.default_rng(3)
    bad_total = 0; control_medians = []

    def oracle_of(e):
        if case == "mu":
            return oracle_cls(robot_model, make(mu=float(held["mu"][e])))
        if case == "kp_kd":
            return oracle_cls(robot_model, make(pd_kp=float(held["kp"][e]), kd=float(held["kd"][e])))
        if case == "plate_mass":
            return oracle_cls(robot_model, make(plate_mass=float(held["plate_mass"][e])))
        mass = np.array(robot_model.mass, dtype=np.float64)
        for s, b in enumerate(order):
            mass[b] = float(held["body_masses"][s, e])
        return oracle_cls(dataclasses.replace(robot_model, mass=mass), make())
    oracles = [oracle_of(e) for e in range(N)]
    for t in range(steps):
        eng.set_phys_env_major(phys); eng.set_task_env_major(task); eng.set_cnt_env_major(cnt)
        act = rng.uniform(-1.0, 1.0, size=(N, 12)).astype(np.float32)
        out = outs(N, ep.num_obs); eng.step(torch.as_tensor(act, device="cuda"), None, *out); torch.cuda.synchronize()
        gobs, gst, grew, grs, gex = [x.cpu().numpy() for x in out]
        goal = np.stack([o0.hash_uniform3(seed, e, int(cnt[e, 5])) for e in range(N)])
        p, tk, c = phys.copy(), task.copy(), cnt.copy()
        obs0, _, _, _ = o0.step(p, tk, c, act.astype(np.float64), goal_rand=goal, seed=seed)
        control_medians.append(float(np.median(np.abs(gobs - np.clip(obs0, -5, 5)).max(1))))
        obs = np.zeros((N, ep.num_obs)); rew = np.zeros(N)
        for e in range(N):
            p, tk, c = phys[e:e + 1].copy(), task[e:e + 1].copy(), cnt[e:e + 1].copy()
            ob, _, rw, _ = oracles[e].step(p, tk, c, act[e:e + 1].astype(np.float64), goal_rand=goal[e:e + 1], seed=seed)
            phys[e], task[e], cnt[e] = p[0], tk[0], c[0]
            obs[e], rew[e] = ob[0], rw[0]
        d = np.abs(gobs - np.clip(obs, -5, 5)).max(1)
        bad = d > 5e-3; bad_total += int(bad.sum()); ok = ~bad
        print(f"[env params] {case} step {t}: median {np.median(d):.3e} max {d.max():.3e} left out {int(bad.sum())} control median {control_medians[-1]:.3e}")
        assert np.median(d) < 3e-4, (t, np.median(d))
        assert np.abs(grew[ok] - rew[ok]).max() < 5e-3 * max(1.0, np.abs(rew).max()), t
    assert bad_total <= 0.02 * steps * N, bad_total
    assert min(control_medians) > 3e-3, control_medians
    # the records report the held values
    rec = {"mu": eng.dr_mu, "body_masses": eng.dr_body_masses, "kp": eng.dr_kp, "kd": eng.dr_kd, "plate_mass": eng.dr_plate_mass}
    for k, v in held.items():
        assert np.array_equal(rec[k].cpu().numpy(), v), k
    eng.close()


# ---- 3. hold wins over a channel; clearing gives the channel back
def test_hold_wins_over_a_channel_and_clearing_gives_it_back(robot_model, engine_cls):
    N = 41          # an odd count: the mask behind the table starts at the next 8-byte boundary
    mass = [DRChannel(), DRChannel(), chan("scaling", "uniform", 0.5, 2.0, 1)]          # body_masses redrawn every step
    dm = [DRChannel(), DRChannel()]; dm[DR_MAT_ROBOT] = DRChannel(enabled=1, operation=DR_OPERATIONS["scaling"], distribution=DR_DISTRIBUTIONS["uniform"], interval=1,
                                                                   p0=[1.0, 0.5, 1.0], p1=[1.0, 1.5, 1.0])          # the feet's material too
    ep = loco_params(dr_enabled=1, dr_mass=mass, dr_mass_body_p0=[0.5] * 21, dr_mass_body_p1=[2.0] * 21, dr_mat=dm)
    eng = engine_cls(robot_model, [ep], N, seed=3)
    eng.enable_env_params()
    held = torch.linspace(0.3, 0.9, N)
    eng.set_env_params(mu=held)
    assert eng.env_params_held == ["mu"]
    g = torch.Generator(device="cuda").manual_seed(1)
    prev = None
    for t in range(4):
        eng.step(torch.rand(N, 12, device="cuda", generator=g) * 2 - 1, None, *outs(N)); torch.cuda.synchronize()
        assert torch.equal(eng.dr_mu.cpu(), held), t          # the held row, every step
        m = eng.dr_mass.clone()
        assert prev is None or not torch.equal(m, prev)          # while the mass channel keeps drawing
        prev = m
    eng.clear_env_params("mu")
    assert eng.env_params_held == []
    mus = []
    for t in range(2):
        eng.step(torch.rand(N, 12, device="cuda", generator=g) * 2 - 1, None, *outs(N)); torch.cuda.synchronize()
        mus.append(eng.dr_mu.cpu().clone())
    for mu in mus:          # the channel's draw again: friction_scale x average(feet x U(0.5, 1.5), ground)
        assert not torch.equal(mu, held) and len(torch.unique(mu)) > N // 2
        assert float(mu.min()) >= ep.friction_scale * 0.5 * (0.5 * ep.mat_mu_robot + ep.mat_mu_other) - 1e-6 and float(mu.max()) <= ep.friction_scale * 0.5 * (1.5 * ep.mat_mu_robot + ep.mat_mu_other) + 1e-6
    assert not torch.equal(mus[0], mus[1])
    eng.close()
    # without a material channel the cleared row is the block's mu again
    eng = engine_cls(robot_model, [loco_params(dr_enabled=1)], N, seed=3)
    eng.enable_env_params(); eng.set_env_params(mu=held, kd=2.0 * loco_params().kd)
    eng.step(torch.zeros(N, 12, device="cuda"), None, *outs(N)); torch.cuda.synchronize()
    assert torch.equal(eng.dr_mu.cpu(), held) and (eng.dr_kd == F32(2.0 * loco_params().kd)).all()
    eng.clear_env_params()
    assert (eng.dr_kd == F32(loco_params().kd)).all()          # a record row no channel writes shows the nominal value again
    eng.step(torch.zeros(N, 12, device="cuda"), None, *outs(N)); torch.cuda.synchronize()
    assert (eng.dr_mu == F32(loco_params().mu)).all() and (eng.dr_kd == F32(loco_params().kd)).all()
    eng.close()


# ---- 4. refusals and neighbours
def test_refusals_leave_the_table_untouched(robot_model, engine_cls):
    from locomanipulationrl_amd.lib import ENV_PARAM_ROWS, PTR_ENV_PARAMS, EngineError, env_param_rows
    N = 32
    plain = engine_cls(robot_model, [loco_params()], N, seed=1)
    assert not plain.lib.lm_ptr(plain._h, PTR_ENV_PARAMS)
    with pytest.raises(EngineError, match="dr_enabled"):
        plain.enable_env_params()
    with pytest.raises(EngineError, match="enable_env_params"):
        plain.set_env_params(mu=0.5)
    with pytest.raises(EngineError, match="enable_env_params"):
        plain.env_params
    v = np.full(N, 0.5, F32)
    assert plain.lib.lm_set_env_params(plain._h, 42, 1, v.ctypes.data_as(C.c_void_p)) == -1 and b"not enabled" in plain.lib.lm_last_error()
    assert plain.lib.lm_clear_env_params(plain._h, 42, 1) == -1 and b"not enabled" in plain.lib.lm_last_error()
    plain.close()
    cf = engine_cls(robot_model, [loco_params(dr_enabled=1)], N, seed=1); cf.enable_contact_forces(True)
    with pytest.raises(EngineError, match="contact-force reporting"):
        cf.enable_env_params()
    cf.enable_contact_forces(False); cf.enable_env_params()          # with reporting off again it goes through ...
    with pytest.raises(EngineError, match="do not combine"):
        cf.enable_contact_forces(True)          # ... and reporting is then refused the same way
    cf.close()

    def refused(eng, why, **named):
        table, mask = eng._env_table().clone(), eng.env_params_mask()
        with pytest.raises(EngineError, match=why):
            eng.set_env_params(**named)
        assert torch.equal(eng._env_table(), table) and np.array_equal(eng.env_params_mask(), mask), named
    loco = engine_cls(robot_model, [loco_params(dr_enabled=1)], N, seed=1); loco.enable_env_params()
    loco.set_env_params(mu=0.7, body_masses=torch.full((21, N), 0.2))
    nan = np.full(N, 0.5, F32); nan[7] = np.nan
    inf = np.full((3, N), 0.0, F32); inf[2, 31] = np.inf
    neg = np.full(N, 0.5, F32); neg[N - 1] = -1e-3
    zero = np.full((21, N), 0.3, F32); zero[20, 0] = 0.0
    refused(loco, "non-finite", mu=nan)
    refused(loco, "non-finite", gravity=inf)
    refused(loco, "must not be negative", mu=neg)
    refused(loco, "must not be negative", max_efforts=-torch.ones(12, N))
    refused(loco, "must not be negative", max_velocities=-torch.ones(12, N))
    refused(loco, "must not be negative", joint_damping=-torch.ones(12, N))
    refused(loco, "must be positive", body_masses=zero)
    refused(loco, "must be positive", kd=0.0)
    refused(loco, "kp row needs a position gain", kp=3.0)
    refused(loco, "latency row exists on the PD-actuator variants", latency=1.0)
    refused(loco, "plate rows exist on engines with a manipulation block only", plate_mass=2.0)
    refused(loco, "plate rows exist on engines with a manipulation block only", plate_inertia_factor=1.0)
    for row0, nrows in ((-1, 1), (ENV_PARAM_ROWS, 1), (60, 10), (0, 0)):
        big = np.ones((max(nrows, 1), N), F32)
        assert loco.lib.lm_set_env_params(loco._h, row0, nrows, big.ctypes.data_as(C.c_void_p)) == -1 and b"rows outside" in loco.lib.lm_last_error()
        assert loco.lib.lm_clear_env_params(loco._h, row0, nrows) == -1 and b"rows outside" in loco.lib.lm_last_error()
    assert loco.lib.lm_set_env_params(loco._h, 42, 1, None) == -1 and b"null" in loco.lib.lm_last_error()
    assert sorted(loco.env_params_held) == ["body_masses", "mu"] and (loco.env_params["mu"] == F32(0.7)).all()
    loco.close()
    eff = engine_cls(robot_model, [loco_params(dr_enabled=1, drive_mode=2, act_scale=1.5)], N, seed=1); eff.enable_env_params()
    refused(eff, "kd row has nothing to act on in effort drive mode", kd=1.0)
    refused(eff, "kp row needs a position gain", kp=1.0)
    eff.close()
    cc = engine_cls(robot_model, [loco_cc_params(dr_enabled=1)], N, seed=1); cc.enable_env_params()
    nsub = loco_cc_params().substeps
    refused(cc, "whole number of sub-steps", latency=1.5)
    refused(cc, "whole number of sub-steps", latency=float(nsub + 1))
    refused(cc, "whole number of sub-steps", latency=-1.0)
    cc.set_env_params(latency=float(nsub), kp=4.0, kd=0.2)          # the whole control period is allowed
    assert sorted(cc.env_params_held) == ["kd", "kp", "latency"] and env_param_rows("latency") == (68, 1)
    cc.step(torch.zeros(N, 12, device="cuda"), None, *outs(N, cc.num_obs)); torch.cuda.synchronize()
    assert (cc.dr_latency == float(nsub)).all() and (cc.dr_kp == 4.0).all() and (cc.dr_kd == F32(0.2)).all() and torch.isfinite(cc.state).all()
    with pytest.raises(EngineError):          # the staged entry points keep refusing randomised engines
        cc.post_physics(torch.zeros(N, 12, device="cuda"))
    cc.close()


@pytest.mark.parametrize("dr", [0, 1])
def test_an_engine_that_never_enables_is_what_it_was(robot_model, engine_cls, dr):
    """Two engines that never opt in - un-randomised (the helper-wavefront kernel) and randomised - beside a third that enables on ANOTHER handle:
    same step_variant, same bits over 4 steps."""
    N = 64
    e1 = engine_cls(robot_model, [loco_params(dr_enabled=dr)], N, seed=9)
    other = engine_cls(robot_model, [loco_params(dr_enabled=1)], N, seed=9); other.enable_env_params(); other.set_env_params(mu=0.3)
    e2 = engine_cls(robot_model, [loco_params(dr_enabled=dr)], N, seed=9)
    assert e1.step_variant == e2.step_variant == ("w1" if dr else "h3") and not e1.env_params_enabled and not e2.env_params_enabled
    g = torch.Generator(device="cuda").manual_seed(5)
    for t in range(4):
        a = torch.rand(N, 12, device="cuda", generator=g) * 2.4 - 1.2
        o1, o2 = outs(N), outs(N)
        e1.step(a, None, *o1); other.step(a, None, *outs(N)); e2.step(a, None, *o2); torch.cuda.synchronize()
        for x, y in zip(o1, o2):
            assert torch.equal(x, y), t
    assert torch.equal(e1.state, e2.state) and torch.equal(e1.cnt, e2.cnt) and torch.equal(e1.dr_mu, e2.dr_mu)
    assert "env_params" not in e1.state_dict()
    for e in (e1, e2, other): e.close()


def test_enabling_recaptures_a_rollout_plan(robot_model, engine_cls):
    """T = 4, 32 envs, MLP: a plan runs once as a graph, then the engine enables env params and holds mu and body masses; the next run("graph")
    equals stepping by hand through the same history with the same held values.  Changing the held values afterwards needs no new plan."""
    from locomanipulationrl_amd.lib import POLICY_MLP, EngineError, Rollout, sample_actions
    from locomanipulationrl_amd.policies.mlp_model import SharedMLP, mlp_forward_hip, pack_mlp_params
    torch.manual_seed(3)
    N, T = 32, 4
    packed = pack_mlp_params(SharedMLP().cuda(), None, None).cuda(); log_std = torch.full((12,), -0.7, device="cuda")
    m = torch.as_tensor(np.asarray([robot_model.mass[k] for k in robot_model.table_body_order()], dtype=np.float32))
    holds = [dict(mu=torch.linspace(0.2, 1.0, N), body_masses=m[:, None] * torch.linspace(0.6, 1.8, N)[None, :]), dict(mu=torch.linspace(1.0, 0.2, N))]
    e1, e2 = (engine_cls(robot_model, [loco_params(dr_enabled=1)], N, seed=4) for _ in range(2))
    obs = []
    for e in (e1, e2):
        o = torch.empty(N, 64, device="cuda"); e.step(torch.zeros(N, 12, device="cuda"), None, o); obs.append(o)
    ro = Rollout(e1, POLICY_MLP, packed, log_std, T, noise_seed=77)
    with pytest.raises(EngineError):
        ro.run("persistent")          # randomised engines never run the persistent kernel
    ro.obs[0] = obs[0]
    hand = obs[1]
    for phase in range(3):
        if phase == 1:
            for e in (e1, e2): e.enable_env_params()
        if phase >= 1:
            for e in (e1, e2): e.set_env_params(**holds[phase - 1])
        ro.run("graph")
        for t in range(T):
            mean, _ = mlp_forward_hip(hand.contiguous(), packed)
            act, _ = sample_actions(e2, mean, log_std, 77)
            o = torch.empty(N, 64, device="cuda"); e2.step(act, None, o); hand = o
        torch.cuda.synchronize()
        assert torch.equal(ro.obs[T], hand) and torch.equal(e1.state, e2.state) and torch.equal(e1.dr_mass, e2.dr_mass), phase
        if phase >= 1:
            assert torch.equal(e1.dr_mu.cpu(), holds[phase - 1]["mu"]), phase          # the re-captured graph launches the kernels that apply the hold
        ro.obs[0].copy_(ro.obs[T])
    ro.close(); e1.close(); e2.close()


def test_state_dict_round_trip(robot_model, engine_cls):
    N = 40
    ep = lambda: mani_params(dr_enabled=1)
    a = engine_cls(robot_model, [ep()], N, seed=6); a.enable_env_params()
    a.set_env_params(plate_mass=torch.linspace(1.0, 3.0, N), mu=torch.linspace(0.3, 1.1, N), gravity=torch.tensor([[0.2], [0.0], [-9.0]]).repeat(1, N), kd=0.7 * ep().kd)
    a.set_env_params(base_force=0.1); a.clear_env_params("base_force")          # a row that was held once: in the table, not in the mask
    g = torch.Generator(device="cuda").manual_seed(2)
    acts = [torch.rand(N, 12, device="cuda", generator=g) * 2 - 1 for _ in range(5)]
    for t in range(2): a.step(acts[t], None, *outs(N))
    sd = a.state_dict()
    assert sd["env_params"]["table"].shape == (69, N) and int(sd["env_params"]["mask"].sum()) == 1 + 1 + 3 + 1
    b = engine_cls(robot_model, [ep()], N, seed=1)          # fresh: not enabled, another seed
    b.load_state_dict(sd)
    assert b.env_params_enabled and sorted(b.env_params_held) == sorted(a.env_params_held) == ["gravity", "kd", "mu", "plate_mass"]
    for t in range(2, 5):
        oa, ob = outs(N), outs(N)
        a.step(acts[t], None, *oa); b.step(acts[t], None, *ob); torch.cuda.synchronize()
        for x, y in zip(oa, ob):
            assert torch.equal(x, y), t
    assert torch.equal(a.state, b.state) and torch.equal(a.cnt, b.cnt) and torch.equal(a.dr_mass, b.dr_mass) and torch.equal(a.dr_phys, b.dr_phys)
    assert (b.dr_plate_mass.cpu() == torch.linspace(1.0, 3.0, N)).all() and (b.dr_phys[26] == -9.0).all()
    c = engine_cls(robot_model, [ep()], N, seed=1)          # a checkpoint without the key loads as before
    sd.pop("env_params"); c.load_state_dict(sd)
    assert not c.env_params_enabled
    for e in (a, b, c): e.close()


# ---- 5. sweep end to end
def test_evaluate_sweep_end_to_end():
    """evaluate() on QuadrupedPoseControl with sim.engine.env_params, 64 envs, mu in 4 levels (env e: level e % 4), an untrained policy, one
    episode per env: the per-group episode counts sum to the total, and the fused and the step-by-step path give equal records."""
    import locomanipulationrl_amd as lm
    from locomanipulationrl_amd.policies.mlp_model import SharedMLP
    from locomanipulationrl_amd.train.evaluate import evaluate, parse_sweep, sweep_env_params, sweep_grid, sweep_groups, sweep_nominals
    from locomanipulationrl_amd.train.ppo import RunningStandardScaler
    torch.manual_seed(14)
    N = 64
    model = SharedMLP().cuda()
    scaler = RunningStandardScaler(64, "cuda"); scaler.update(torch.randn(256, 64, device="cuda") * 0.5)
    points = sweep_grid([parse_sweep("mu=0.2:1.1:4")]); groups = sweep_groups(N, len(points))
    res = []
    for fused in (True, False):
        env = lm.make_env("QuadrupedPoseControl", num_envs=N, seed=3, overrides={"task": {"sim": {"max_episode_length": 20, "engine": {"env_params": True}}}})
        task = env._task
        assert task.engine.env_params_enabled and task.engine.step_variant == "w1" and not task.randomize_observations and not task.randomize_actions
        held = sweep_env_params(points, groups, **sweep_nominals(task))
        res.append(evaluate(env, model, scaler, episodes_per_env=1, max_steps=48, deterministic=True, fused=fused, return_record=True,
                            env_params=held, groups=torch.as_tensor(groups)))
        assert np.array_equal(task.engine.dr_mu.cpu().numpy(), held["mu"]) and task.engine.env_params_held == ["mu"]
        env.close()
    a, b = res
    assert torch.equal(a["record"], b["record"])
    for out in res:
        assert sorted(out["groups"]) == [0, 1, 2, 3]
        assert sum(g["episodes"] for g in out["groups"].values()) == out["episodes"] == N and out["envs_short"] == 0
        for k, g in out["groups"].items():
            assert g["episodes"] == N // 4 and g["goals"] + g["timeouts"] + g["failures"] == g["episodes"]
    assert a["groups"] == b["groups"]
