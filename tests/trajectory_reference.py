"""Independent numpy reference of the trajectory record (include/lm_policy.h): the layout table and the update rule, written from the
specification, not from the kernel.  A record is (rows float32 [K][max_rows][64], header int32 [K][4] = rows written, episodes completed,
rows dropped, 0)."""
import numpy as np

COLS = 64
# state rows: base pose 0..6, q 13, qd 25, plate pose 37..43, last actions 50, last tips 74, goal 86
FB0, Q, QD, FB1, LACT, LTIP, GOAL = 0, 13, 25, 37, 50, 74, 86
GOAL_RESET, PROGRESS, EPISODE_COUNT = 2, 4, 5          # counter rows
ROWS, EPISODES, DROPPED = 0, 1, 2                      # header words


def new_record(K, max_rows):
    return np.zeros((K, max_rows, COLS), np.float32), np.zeros((K, 4), np.int32)


def row_of(state, cnt, rewards, dones, env, manipulation):
    """The 64 columns for one env after a step.  state (115, N) float32, cnt (6, N) int64, rewards (N,), dones (N,)."""
    r = np.zeros(COLS, np.float32)
    fb = FB1 if manipulation else FB0
    r[0:12] = state[Q:Q + 12, env]
    r[12:24] = state[QD:QD + 12, env]
    r[24:31] = state[fb:fb + 7, env]
    r[31:43] = state[LACT:LACT + 12, env]
    r[43:55] = state[LTIP:LTIP + 12, env]
    r[55:59] = state[GOAL:GOAL + 4, env]
    r[59] = np.float32(rewards[env])
    r[60] = 1.0 if dones[env] != 0 else 0.0
    r[61] = 1.0 if cnt[GOAL_RESET, env] != 0 else 0.0
    r[62] = np.float32(cnt[PROGRESS, env])
    r[63] = np.float32(cnt[EPISODE_COUNT, env])
    return r


def update(rows, header, state, cnt, rewards, dones, env_ids, manipulation, cap=1):
    """One step.  manipulation[k]: slot k tracks an env of a manipulation block (the free body is the plate)."""
    state, cnt, rewards, dones = (np.asarray(x) for x in (state, cnt, rewards, dones))
    max_rows = rows.shape[1]
    for k, env in enumerate(env_ids):
        if cap > 0 and header[k, EPISODES] >= cap:
            continue
        if header[k, ROWS] < max_rows:
            rows[k, header[k, ROWS]] = row_of(state, cnt, rewards, dones, env, manipulation[k])
            header[k, ROWS] += 1
        else:
            header[k, DROPPED] += 1
        if dones[env] != 0:
            header[k, EPISODES] += 1
    return rows, header


def same_bits(a, b):
    """Exact equality of two float32 arrays, NaNs included (the record is a copy)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
