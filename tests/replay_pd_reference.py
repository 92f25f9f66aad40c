"""Float32 numpy restatement of the replay rule for PD-actuator plans of include/lm_policy.h ("PD-actuator engines: lm_replay_create_pd"),
written from the header text: what k_replay_update_pd and the PD branch of ReplayRecord's torch path are compared with, bit for bit.
TEST INFRASTRUCTURE.

One env at a time, plain Python in the order the header writes the rule, every operation on np.float32 values so that each result is rounded
where the device rounds it (no contraction: a product and the sum it feeds are two operations).  The record is a (32, N) float32 array with the
header's rows."""
import numpy as np

F = np.float32
ROWS = 32
(ROWS_, FINISHED, DONE_AT, GOAL, ROW0_ERR, QERR, SQ_SUM, TRACKED, EARLY, FIRST_SUCC, IN_WINDOW, MIN_V2, RET, WINDOW_RETURN, V2_FIRST, ABS_SUM, QPREV) = range(17)
SATURATED, CMD_ERR = 28, 29
CMD_ACTIONS, CMD_TARGETS = 0, 1


def zero_record(N):
    rec = np.zeros((ROWS, N), dtype=F); rec[DONE_AT] = -1.0; rec[FIRST_SUCC] = -1.0; rec[MIN_V2] = np.inf
    return rec


def se_command(t):
    """Joint position targets (joint order of rec) -> the swing / extension command: rows l dof1, 4+2l swing, 5+2l extension."""
    t = np.asarray(t, dtype=F); c = np.zeros(12, dtype=F)
    for l in range(4):
        c[l] = t[l]
        c[4 + 2 * l] = F(0.5) * (t[4 + 2 * l] + t[5 + 2 * l])
        c[5 + 2 * l] = t[4 + 2 * l] - t[5 + 2 * l]
    return c


def joint_targets(se):
    """The step's own map (lm_step.h tgtq), the one se_command inverts: dof1, dof2 = swing + extension / 2, dof3 = swing - extension / 2."""
    se = np.asarray(se, dtype=F); t = np.zeros(12, dtype=F)
    for l in range(4):
        t[l] = se[l]
        t[4 + 2 * l] = se[4 + 2 * l] + F(0.5) * se[5 + 2 * l]
        t[5 + 2 * l] = se[4 + 2 * l] - F(0.5) * se[5 + 2 * l]
    return t


def seq_sum(x):
    """j = 0 .. 11 from zero, in order."""
    acc = F(0.0)
    for v in x:
        acc = F(acc + v)
    return acc


class Plan:
    """The tables of a PD plan on the host: rec / cmd (R, T_max, 12), lens (R,), env_rec (N,), the scalars of lm_replay_create_pd and what the
    plan reads from the engine's blocks, per env: the variant and the float reciprocal of the action scale (1 / act_scale_se for variants 1 / 2,
    1 / act_scale for variant 0)."""

    def __init__(self, rec, cmd, lens, env_rec, cmd_mode, hold, window_rows, v2_thresh, track_tol, variant, scale):
        self.rec, self.cmd = np.asarray(rec, dtype=F), np.asarray(cmd, dtype=F)
        self.lens, self.env_rec = np.asarray(lens, dtype=np.int64), np.asarray(env_rec, dtype=np.int64)
        self.cmd_mode, self.hold, self.window_rows = int(cmd_mode), int(hold), int(window_rows)
        self.v2_thresh, self.track_tol = F(v2_thresh), F(track_tol)
        self.variant = np.asarray(variant, dtype=np.int64)
        self.inv_scale = F(1.0) / np.asarray(scale, dtype=F)          # formed once, in float

    def steps(self):
        used = self.env_rec[self.env_rec >= 0]
        return int(max((self.lens[r] + self.hold for r in used), default=0))


def update(plan, record, s, q, se, obs, rewards, goal_flag, reset_flag):
    """After step s: q (12, N) state rows R_Q, se (12, N) state rows R_SE, obs (N, width), rewards (N,), goal_flag / reset_flag (N,) =
    LM_PTR_CNT rows 2 / 3.  Updates `record` in place and returns actions_next (N, 12) float32."""
    assert record.dtype == F
    N = record.shape[1]
    nxt = np.zeros((N, 12), dtype=F)
    targets = plan.cmd_mode == CMD_TARGETS
    for e in range(N):
        r = int(plan.env_rec[e])
        if r < 0:
            continue
        T = int(plan.lens[r]); R = record[:, e]
        if R[FINISHED] != 0 or s >= T + plan.hold:
            continue
        qe = np.asarray(q[:, e], dtype=F); o = np.asarray(obs[e], dtype=F); rew = F(rewards[e])
        see = np.asarray(se[:, e], dtype=F)
        v2 = F(F(F(o[7] * o[7]) + F(o[8] * o[8])) + F(o[9] * o[9]))
        pd_cmd = targets and plan.variant[e] >= 1
        if s < T:
            d = qe - plan.rec[r, s]; ad = np.abs(d); m = ad.max()
            if s == 0:
                R[ROW0_ERR] = m; R[V2_FIRST] = v2
            R[QERR] = max(R[QERR], m); R[ABS_SUM] = F(R[ABS_SUM] + seq_sum(ad)); R[SQ_SUM] = F(R[SQ_SUM] + seq_sum(d * d))
            if s >= 1:
                ej = np.abs((qe - R[QPREV:QPREV + 12]) - (plan.rec[r, s] - plan.rec[r, s - 1]))
                R[TRACKED] = F(R[TRACKED] + F(int((ej < plan.track_tol).sum())))
                if s <= 4:
                    R[EARLY] = F(R[EARLY] + seq_sum(ej))
                if pd_cmd:
                    R[CMD_ERR] = max(R[CMD_ERR], np.abs(se_command(plan.cmd[r, s]) - see).max())
            win = s >= T - plan.window_rows
            if v2 <= plan.v2_thresh:
                if R[FIRST_SUCC] < 0:
                    R[FIRST_SUCC] = s
                if win:
                    R[IN_WINDOW] = F(R[IN_WINDOW] + F(1.0))
            R[MIN_V2] = min(R[MIN_V2], v2)
            if win:
                R[WINDOW_RETURN] = F(R[WINDOW_RETURN] + rew)
            R[ROWS_] = F(R[ROWS_] + F(1.0)); R[QPREV:QPREV + 12] = qe
        R[RET] = F(R[RET] + rew)
        if reset_flag[e] != 0:
            R[FINISHED] = 1; R[DONE_AT] = s; R[GOAL] = 1.0 if goal_flag[e] != 0 else 0.0
        if R[FINISHED] == 0 and s + 1 < T:
            t = plan.cmd[r, s + 1]
            if not targets:
                nxt[e] = t
            else:
                raw = (se_command(t) - see) * plan.inv_scale[e] if plan.variant[e] >= 1 else t * plan.inv_scale[e]
                raw = np.asarray(raw, dtype=F)
                R[SATURATED] = F(R[SATURATED] + F(int((np.abs(raw) > F(1.0)).sum())))
                nxt[e] = np.minimum(np.maximum(raw, F(-1.0)), F(1.0))
    return nxt
