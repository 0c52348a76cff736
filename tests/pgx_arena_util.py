"""The arena's contract (envpool_amd/csrc/pgx_arena.hip.h) restated in numpy: which net moves, the plan, the wave
mapping, the tally of seven, and the side patterns the tests share."""
import numpy as np

import pgx_selfplay_util as SU

WAVE = 64


def net_of(env_id, seat):
    return (np.asarray(seat) ^ np.asarray(env_id)) & 1


def plan(side):
    """(order int32 [rows], n0): the stable partition of the row indices by side."""
    side = np.asarray(side).reshape(-1)
    order = np.argsort(side != 0, kind="stable").astype(np.int32)
    return order, int((side == 0).sum())


def waves(rows):
    return -(-rows // WAVE) + 1


def wave_map(rows, n0):
    """int32 [waves(rows), 3]: (net, first entry, entries) of every launched wave."""
    out = np.zeros((waves(rows), 3), np.int32)
    w0 = -(-n0 // WAVE)
    for b in range(waves(rows)):
        if b < w0:
            out[b] = (0, WAVE * b, min(WAVE, n0 - WAVE * b))
        else:
            at = WAVE * (b - w0)
            out[b] = (1, n0 + at, max(0, min(WAVE, rows - n0 - at)))
    return out


def tally(done, reward, elapsed, env_ids):
    """What a step's results add to (games, wins0, wins1, draws, plies, wins_a, wins_b)."""
    d = np.asarray(done).astype(bool).reshape(-1)
    r = np.asarray(reward, np.float32).reshape(-1, 2)
    seat_a = np.asarray(env_ids).reshape(-1) & 1
    rows = np.arange(len(d))
    ra, rb = r[rows, seat_a], r[rows, 1 - seat_a]
    return np.concatenate([SU.tally(done, reward, elapsed),
                           np.array([(d & (ra > 0)).sum(), (d & (rb > 0)).sum()], dtype=np.int64)])


def side_patterns(rows, seed=0):
    """name -> uint8 [rows]: all 0, all 1, alternating, 0-then-1, 1-then-0, random, and n0 in {0, 1, 63, 64, 65, rows}
    (scattered by a fixed permutation, where rows allows it)."""
    rng = np.random.default_rng(seed + rows)
    i = np.arange(rows)
    out = {"all0": np.zeros(rows, np.uint8), "all1": np.ones(rows, np.uint8), "alternating": (i & 1).astype(np.uint8),
           "0then1": (i >= rows // 2).astype(np.uint8), "1then0": (i < rows // 2).astype(np.uint8),
           "random": rng.integers(0, 2, rows).astype(np.uint8)}
    for n0 in (0, 1, 63, 64, 65, rows):
        if n0 <= rows:
            s = np.ones(rows, np.uint8)
            s[rng.permutation(rows)[:n0]] = 0
            out[f"n0={n0}"] = s
    return out
