"""Independent reference for the episode record (include/lm_policy.h, lm_rollout_set_episode_record): a plain numpy loop over per-step
(rewards, dones, goal flag) streams, sequential per env, every add in np.float32 in step order.  TEST USE ONLY.

The rule, per env after step t with r = rewards[t], d = dones[t], g = the env's goal flag after that step, M = max_episode of its block:
    if cap > 0 and row2 >= cap: skip the env
    row0 = row0 + r; row1 = row1 + 1
    if d: row2 += 1; row3 = row3 + row0; row4 = row4 + row1; (row5 if g else row6 if row1 >= M - 1 else row7) += 1; row8 = row0; row0 = row1 = 0
Because these are plain fp32 adds in a fixed order, implementations are compared with exact equality on all nine rows."""
import numpy as np

ROWS = 9
RUN_RETURN, RUN_LENGTH, EPISODES, SUM_RETURN, SUM_LENGTH, GOAL, TIMEOUT, FAILURE, LAST_RETURN = range(ROWS)


def new_record(n_envs):
    return np.zeros((ROWS, n_envs), np.float32)


def update(record, rewards, dones, goals, max_episode, cap=0):
    """Apply the steps rewards / dones / goals [T][N] (or [N] for one step) to `record` [9][N] in place; max_episode: int or per-env [N]."""
    rewards = np.atleast_2d(np.asarray(rewards, np.float32)); dones = np.atleast_2d(np.asarray(dones)); goals = np.atleast_2d(np.asarray(goals))
    T, N = rewards.shape
    assert record.shape == (ROWS, N) and record.dtype == np.float32 and dones.shape == (T, N) and goals.shape == (T, N)
    M = np.broadcast_to(np.asarray(max_episode), (N,))
    one = np.float32(1.0)
    for e in range(N):
        col = record[:, e]
        for t in range(T):
            if cap > 0 and col[EPISODES] >= cap:
                break
            col[RUN_RETURN] = np.float32(col[RUN_RETURN] + rewards[t, e])
            col[RUN_LENGTH] = np.float32(col[RUN_LENGTH] + one)
            if dones[t, e] != 0:
                col[EPISODES] = np.float32(col[EPISODES] + one)
                col[SUM_RETURN] = np.float32(col[SUM_RETURN] + col[RUN_RETURN])
                col[SUM_LENGTH] = np.float32(col[SUM_LENGTH] + col[RUN_LENGTH])
                how = GOAL if goals[t, e] != 0 else (TIMEOUT if col[RUN_LENGTH] >= M[e] - 1 else FAILURE)
                col[how] = np.float32(col[how] + one)
                col[LAST_RETURN] = col[RUN_RETURN]
                col[RUN_RETURN] = np.float32(0.0); col[RUN_LENGTH] = np.float32(0.0)
    return record


def tallies(record):
    """(episodes, goals, timeouts, failures) summed over the envs."""
    return tuple(int(record[r].sum()) for r in (EPISODES, GOAL, TIMEOUT, FAILURE))
