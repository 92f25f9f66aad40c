"""Float64 numpy restatement of the replay rule of include/lm_policy.h ("replay of recorded joint motions"), written from the header text:
what lm_replay_update and ReplayRecord's torch path are compared with.  TEST INFRASTRUCTURE.

One env at a time, plain Python in the order the header writes the rule; the record is a (32, N) float64 array with the header's rows."""
import numpy as np

ROWS = 32
(ROWS_, FINISHED, DONE_AT, GOAL, ROW0_ERR, QERR, SQ_SUM, TRACKED, EARLY, FIRST_SUCC, IN_WINDOW, MIN_V2, RET, WINDOW_RETURN, V2_FIRST, ABS_SUM, QPREV) = range(17)
INTEGER_ROWS = (ROWS_, FINISHED, DONE_AT, GOAL, TRACKED, FIRST_SUCC, IN_WINDOW)
FLOAT_ROWS = (ROW0_ERR, QERR, SQ_SUM, EARLY, MIN_V2, RET, WINDOW_RETURN, V2_FIRST, ABS_SUM) + tuple(range(QPREV, QPREV + 12))


def zero_record(N):
    rec = np.zeros((ROWS, N)); rec[DONE_AT] = -1.0; rec[FIRST_SUCC] = -1.0; rec[MIN_V2] = np.inf
    return rec


class Plan:
    """The tables of a replay plan on the host: rec / act (R, T_max, 12), lens (R,), env_rec (N,) and the scalars of lm_replay_create."""

    def __init__(self, rec, act, lens, env_rec, servo, hold, window_rows, inv_full, v2_thresh, track_tol):
        self.rec, self.act = np.asarray(rec, dtype=np.float64), np.asarray(act, dtype=np.float64)
        self.lens, self.env_rec = np.asarray(lens, dtype=np.int64), np.asarray(env_rec, dtype=np.int64)
        self.servo, self.hold, self.window_rows = bool(servo), int(hold), int(window_rows)
        self.inv_full, self.v2_thresh, self.track_tol = float(inv_full), float(v2_thresh), float(track_tol)

    def steps(self):
        used = self.env_rec[self.env_rec >= 0]
        return int(max((self.lens[r] + self.hold for r in used), default=0))


def update(plan, record, s, q, obs, rewards, goal_flag, reset_flag):
    """After step s: q (12, N) state rows R_Q, obs (N, 64), rewards (N,), goal_flag / reset_flag (N,) = LM_PTR_CNT rows 2 / 3.  Updates `record`
    in place and returns actions_next (N, 12)."""
    N = record.shape[1]
    nxt = np.zeros((N, 12))
    for e in range(N):
        r = int(plan.env_rec[e])
        if r < 0:
            continue
        T = int(plan.lens[r]); R = record[:, e]
        if R[FINISHED] != 0 or s >= T + plan.hold:
            continue
        qe = np.asarray(q[:, e], dtype=np.float64); o = np.asarray(obs[e], dtype=np.float64); rew = float(rewards[e])
        v2 = (o[7] * o[7] + o[8] * o[8]) + o[9] * o[9]
        if s < T:
            d = qe - plan.rec[r, s]; m = np.abs(d).max()
            if s == 0:
                R[ROW0_ERR] = m; R[V2_FIRST] = v2
            R[QERR] = max(R[QERR], m); R[ABS_SUM] += np.abs(d).sum(); R[SQ_SUM] += (d * d).sum()
            if s >= 1:
                ej = (qe - R[QPREV:QPREV + 12]) - (plan.rec[r, s] - plan.rec[r, s - 1])
                R[TRACKED] += int((np.abs(ej) < plan.track_tol).sum())
                if s <= 4:
                    R[EARLY] += np.abs(ej).sum()
            if v2 <= plan.v2_thresh:
                if R[FIRST_SUCC] < 0:
                    R[FIRST_SUCC] = s
                if s >= T - plan.window_rows:
                    R[IN_WINDOW] += 1
            R[MIN_V2] = min(R[MIN_V2], v2)
            if s >= T - plan.window_rows:
                R[WINDOW_RETURN] += rew
            R[ROWS_] += 1; R[QPREV:QPREV + 12] = qe
        R[RET] += rew
        if reset_flag[e] != 0:
            R[FINISHED] = 1; R[DONE_AT] = s; R[GOAL] = 1.0 if goal_flag[e] != 0 else 0.0
        if R[FINISHED] == 0 and s + 1 < T:
            nxt[e] = np.clip((plan.rec[r, s + 1] - qe) * plan.inv_full, -1.0, 1.0) if plan.servo else plan.act[r, s + 1]
    return nxt


def margins(plan, record, s, q, obs):
    """The distances of this step's threshold comparisons from their thresholds, BEFORE update(plan, record, s, ...) is applied: (smallest
    | |e_j| - track_tol | over the envs and joints compared, smallest | v2 - v2_thresh |); inf where nothing is compared.  A test that demands
    exact integer rows of an fp32 implementation keeps both above the fp32 error of the compared quantities."""
    mt, mv = np.inf, np.inf
    for e in range(record.shape[1]):
        r = int(plan.env_rec[e])
        if r < 0 or record[FINISHED, e] != 0 or s >= plan.lens[r]:
            continue
        o = np.asarray(obs[e], dtype=np.float64)
        mv = min(mv, abs((o[7] * o[7] + o[8] * o[8]) + o[9] * o[9] - plan.v2_thresh))
        if s >= 1:
            ej = (np.asarray(q[:, e], dtype=np.float64) - record[QPREV:QPREV + 12, e]) - (plan.rec[r, s] - plan.rec[r, s - 1])
            mt = min(mt, np.abs(np.abs(ej) - plan.track_tol).min())
    return mt, mv


def summary(record, full):
    """The quantities of npy_replay.replay() per env from a record (float64 arrays of shape (N,)); what ReplayRecord.summary() returns."""
    rec = np.asarray(record, dtype=np.float64); rows = rec[ROWS_]; steps = np.maximum(rows - 1.0, 0.0)
    rd = lambda v2: 2.0 * np.arcsin(np.sqrt(np.clip(v2, 0.0, 1.0)))
    with np.errstate(divide="ignore", invalid="ignore"):
        out = dict(rows=rows.astype(np.int64), finished=rec[FINISHED] != 0, done_at=rec[DONE_AT].astype(np.int64), goal=rec[GOAL].astype(np.int64),
                   row0_err=rec[ROW0_ERR], qerr=rec[QERR], rms=np.sqrt(rec[SQ_SUM] / (12.0 * rows)), mean_abs=rec[ABS_SUM] / (12.0 * rows),
                   tracked=rec[TRACKED] / (12.0 * steps), early=rec[EARLY] / (12.0 * np.minimum(4.0, steps) * full), first_succ=rec[FIRST_SUCC].astype(np.int64),
                   in_window=rec[IN_WINDOW].astype(np.int64), min_rd=rd(rec[MIN_V2]), rd_first=rd(rec[V2_FIRST]), window_return=rec[WINDOW_RETURN])
    out["return"] = rec[RET]
    return out
