"""The PGX self-play recorder's contract (envpool_amd/csrc/pgx_record.hip.h) restated in numpy, and what the recorder
tests share: the test policy, the replay of a fixture through a recorder of any kind, and the samples a fixture holds.

The restatement shares no code with the header: it never sees a position, only the observation and mask rows of the
fixture (or of a pool's recv), and its symmetries are numpy's own rot90 / transpose / flips of the [H, W] board."""
import numpy as np

from pgx_util import ACTIONS, fixture, game

F = np.float32
FIELDS = ("obs", "mask", "policy", "value", "ply", "env_id", "sym")
NSYM = {"TicTacToe": 8, "ConnectFour": 2, "Hex": 2, "Othello": 8}
# finished games and their plies in the whole fixtures, counted once from the fixtures themselves (test_pgx_record_host
# asserts them): TicTacToe, ConnectFour, Hex, Othello
GAMES = {"TicTacToe-v1": (191, 1084), "ConnectFour-v1": (303, 5196), "Hex-v1": (48, 3565), "Othello-v1": (137, 6859)}
TRUNC_GAMES = {"TicTacToe-v1__trunc": 16, "ConnectFour-v1__trunc": 13, "Hex-v1__trunc": 3, "Othello-v1__trunc": 8}
# the scripted fixtures: (finished games, their plies), the fixtures' done rows and the elapsed steps at them
SCRIPTED_GAMES = {"TicTacToe-v1__scripted": (20, 121), "ConnectFour-v1__scripted": (79, 1814),
                  "Hex-v1__scripted": (39, 314), "Othello-v1__scripted": (14, 586)}


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def policy_rows(name, t, n, lo=0):
    """The test policy of envs lo .. lo + n - 1 at fixture row t: a seeded float32 row per (env, t) with NaN, +-inf,
    negative numbers and non-zero entries on illegal actions mixed in (the rows of an env do not depend on n)."""
    a = ACTIONS[game(name)]
    out = np.empty((n, a), F)
    for i in range(n):
        rng = np.random.default_rng([len(name), t, lo + i])
        p = (rng.random(a) * 2 - 0.5).astype(F)
        u = rng.random(a)
        p[u < 0.06] = np.nan
        p[(u >= 0.06) & (u < 0.09)] = np.inf
        p[(u >= 0.09) & (u < 0.12)] = -np.inf
        out[i] = p
    return out


def sym_board(gm, j, x):
    """sigma_j of an array whose two leading axes are the board's [H, W]: the value at a cell moves to sigma_j(cell)."""
    if j == 0:
        return x
    if gm in ("TicTacToe", "Othello"):
        if j >= 4:
            x = np.swapaxes(x, 0, 1)  # (r, c) -> (c, r)
        return np.rot90(x, -(j & 3), axes=(0, 1))  # clockwise: (r, c) -> (c, n - 1 - r), j & 3 times
    if gm == "ConnectFour":
        return x[:, ::-1]
    return x[::-1, ::-1]  # Hex


def sym_actions(gm, j, row):
    """sigma_j of a per-action row (mask, policy)."""
    if gm == "ConnectFour":
        return row[::-1] if j else row
    h, w = {"TicTacToe": (3, 3), "Hex": (11, 11), "Othello": (8, 8)}[gm]
    cells = sym_board(gm, j, row[:h * w].reshape(h, w)).reshape(-1)
    return np.concatenate([cells, row[h * w:]])  # Othello's pass, Hex's swap: fixed


class Model:
    """The recorder, restated.  add / finish take the rows the caller reads off the fixture or the pool."""

    def __init__(self, gm, n_envs, capacity, max_plies=0, symmetries=False, id_offset=0):
        self.gm, self.capacity, self.id_offset = gm, capacity, id_offset
        self.plies = 128 if max_plies == 0 else max_plies
        self.nsym = NSYM[gm] if symmetries else 1
        self.staged = [[] for _ in range(n_envs)]
        self.rows = []
        self.counters = dict(samples=0, games=0, dropped_games=0, dropped_plies=0)

    def add(self, ids, over, elapsed, mover, obs, mask, policy):
        """Row i, env ids[i] (local): the env is over [k], its elapsed step [k], the seat to move [k], that seat's obs
        [k, H, W, C], the mask [k, A] and the caller's policy [k, A]."""
        for i, e in enumerate(ids):
            if over[i]:
                continue
            st = self.staged[e]
            if len(st) > elapsed[i]:  # an abandoned game
                self.counters["dropped_games"] += 1
                self.counters["dropped_plies"] += len(st)
                st.clear()
            if len(st) == self.plies:
                self.counters["dropped_plies"] += 1
                continue
            pb = bits(policy[i]).copy()
            keep = mask[i].astype(bool) & np.isfinite(policy[i])
            pb[~keep] = 0
            st.append((obs[i].astype(np.uint8), mask[i].astype(np.uint8), pb, int(elapsed[i]), int(mover[i])))

    def finish(self, ids, reward, done):
        reward = bits(np.asarray(reward, F).reshape(len(ids), 2))
        base, off = len(self.rows), 0
        for i, e in enumerate(ids):
            if not done[i]:
                continue
            st, self.staged[e] = self.staged[e], []
            c = len(st) * self.nsym
            if c == 0:
                continue
            fits = base + off + c <= self.capacity
            off += c
            if not fits:
                self.counters["dropped_games"] += 1
                self.counters["dropped_plies"] += len(st)
                continue
            self.counters["games"] += 1
            self.counters["samples"] += c
            for obs, mask, pol, el, mover in st:
                for j in range(self.nsym):
                    self.rows.append((sym_board(self.gm, j, obs), sym_actions(self.gm, j, mask),
                                      sym_actions(self.gm, j, pol), reward[i, mover], el, e + self.id_offset, j))

    def discard(self, ids):
        for e in ids:
            self.staged[e] = []

    def drain(self):
        rows, self.rows = self.rows, []
        return stack(rows, self.gm)


def stack(rows, gm):
    """A list of sample tuples as the seven arrays (policy and value as uint32 bit patterns)."""
    a = ACTIONS[gm]
    h, w, c = {"TicTacToe": (3, 3, 2), "ConnectFour": (6, 7, 2), "Hex": (11, 11, 4), "Othello": (8, 8, 2)}[gm]
    n = len(rows)
    cols = list(zip(*rows)) if n else [[]] * 7
    return (np.array(cols[0], np.uint8).reshape(n, h, w, c), np.array(cols[1], np.uint8).reshape(n, a),
            np.array(cols[2], np.uint32).reshape(n, a), np.array(cols[3], np.uint32).reshape(n),
            np.array(cols[4], np.int32).reshape(n), np.array(cols[5], np.int32).reshape(n),
            np.array(cols[6], np.uint8).reshape(n))


def as_bits(samples):
    """Seven arrays as a recorder returns them (bool / float32) in the form `stack` gives."""
    o, m, p, v, ply, env, sym = samples
    return (np.asarray(o).astype(np.uint8), np.asarray(m).astype(np.uint8), bits(p), bits(v),
            np.asarray(ply, np.int32), np.asarray(env, np.int32), np.asarray(sym, np.uint8))


def assert_same(got, want, where):
    got, want = as_bits(got) if got[2].dtype != np.uint32 else got, want
    for name, x, y in zip(FIELDS, got, want):
        assert x.shape == y.shape, (where, name, x.shape, y.shape)
        assert np.array_equal(x, y), (where, name, int(np.flatnonzero((x != y).reshape(len(x), -1).any(1))[0]))


def fixture_samples(name, steps=None, envs=None, id_offset=0):
    """The samples a fixture holds, straight from its arrays (no symmetries), in the order of a recorder that is given
    every env in id order at every step: per step the games that ended, by env; per game its plies.  Returns the seven
    arrays and (games, plies)."""
    g = fixture(name)
    gm = game(name)
    t_max = len(g["actions"]) if steps is None else steps
    n = g["done"].shape[1] if envs is None else envs
    staged = [[] for _ in range(n)]
    rows, games, plies = [], 0, 0
    for t in range(t_max):
        pol = policy_rows(name, t, n)
        for e in range(n):
            if g["done"][t, e]:
                continue
            cp = int(g["info:current_player"][t, e])
            m = g["info:legal_action_mask"][t, e]
            pb = bits(pol[e]).copy()
            pb[~(m & np.isfinite(pol[e]))] = 0
            staged[e].append((g["obs"][t, e, cp].astype(np.uint8), m.astype(np.uint8), pb,
                              int(g["elapsed_step"][t, e]), cp))
        for e in range(n):
            if g["done"][t + 1, e] and staged[e]:
                games += 1
                plies += len(staged[e])
                for obs, m, pb, el, cp in staged[e]:
                    rows.append((obs, m, pb, bits(g["reward"][t + 1, e])[cp], el, e + id_offset, 0))
                staged[e] = []
    return stack(rows, gm), (games, plies)
