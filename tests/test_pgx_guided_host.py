"""PGX guided tree search, CPU side: the stepwise search of envpool_amd/csrc/pgx_guided.hip.h built for the host by g++
(a harness that walks a wave's lanes as loops) against the contract restated in numpy (pgx_guided_util.py), which keeps
the tree in Python, takes every position, observation and expansion step from the reference-pinned `pgx_replay` of the
PGX host harness and shares no code with the header; and the argument checks of the Python wrappers, which come before
any native call."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from pgx_guided_util import GuidedTree, Pos, stand_in
from pgx_util import ACTIONS, CODE, KEYS, fixture, game

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMES = ["TicTacToe-v1", "ConnectFour-v1", "Hex-v1", "Othello-v1"]
S = 24
F = np.float32


def _build(tmp, source, name):
    out = str(tmp / name)
    # no fast-math, no contraction: the score is float32, operation by operation
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "cpu_harness", source), "-o", out], check=True)
    return ctypes.CDLL(out)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pgx_guided")
    guided = _build(tmp, "pgx_guided_host.cpp", "libpgxguidedhost.so")
    guided.pgx_guided_begin.restype = ctypes.c_void_p
    guided.pgx_guided_result.restype = None
    guided.pgx_guided_end.restype = None
    return _build(tmp, "pgx_host.cpp", "libpgxhost.so"), guided


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Replayed:
    """Positions of one env column of a fixture, named by their action sequence from the reset (pgx_replay)."""

    def __init__(self, libs, tid, column):
        self.host = libs[0]
        self.tid, self.code = tid, CODE[game(tid)]
        self.g = fixture(tid)
        self.column = column
        self.words = self.host.pgx_hidden_words(self.code)
        self.expanded = []

    def at(self, seq):
        """The position after the actions `seq` from the column's reset, and the step rewards that led to it."""
        seq = [int(a) for a in seq]
        acts = np.array(seq, np.int32).reshape(len(seq), 1)
        outs = {k: np.zeros((len(seq) + 1, 1) + self.g[k].shape[2:], self.g[k].dtype) for k in KEYS}
        hid = np.zeros((len(seq) + 1, 1, self.words), np.int32)
        ptrs = (ctypes.c_void_p * len(KEYS))(*[outs[k].ctypes.data for k in KEYS])
        seeds = np.array([int(self.g["seed"]) + self.column], np.int32)
        assert self.host.pgx_replay(self.code, 1, len(seq), _ptr(seeds), _ptr(acts), 2**31 - 1, ptrs, _ptr(hid)) == 0
        mover = int(outs["info:current_player"][-1, 0])
        pos = Pos(mask=outs["info:legal_action_mask"][-1, 0].astype(bool), done=bool(outs["done"][-1, 0]), mover=mover,
                  obs=outs["obs"][-1, 0, mover].astype(bool), key=(tuple(seq), hid[-1, 0].copy()))
        return pos, outs["reward"][-1, 0]

    def fixture_row(self, t0):
        return self.at(self.g["actions"][:t0, self.column])[0]

    def expand(self, pos, a):
        assert pos.mask[a] and not pos.done
        new, rw = self.at(pos.key[0] + (a,))
        assert rw[0] == -rw[1] and rw[0] in (-1.0, 0.0, 1.0)  # zero-sum
        assert new.done or rw[0] == 0
        self.expanded.append(a)
        return new, int(rw[0])


class HostSession:
    """The harness's session over the roots `poss` (Pos with key = (seq, hidden words))."""

    def __init__(self, libs, tid, poss, simulations, c_puct):
        self.lib, self.n, self.n_act = libs[1], len(poss), ACTIONS[game(tid)]
        hid = np.ascontiguousarray(np.stack([p.key[1] for p in poss]), np.int32)
        done = np.array([p.done for p in poss], np.uint8)
        self.obs = np.full((self.n,) + poss[0].obs.shape, 7, np.uint8)
        self.mask = np.full((self.n, self.n_act), 7, np.uint8)
        self.status = np.full(self.n, 7, np.uint8)
        rc = ctypes.c_int(-9)
        self.h = self.lib.pgx_guided_begin(CODE[game(tid)], self.n, _ptr(hid), _ptr(done), simulations,
                                           ctypes.c_float(c_puct), _ptr(self.obs), _ptr(self.mask), _ptr(self.status),
                                           ctypes.byref(rc))
        assert rc.value == 0 and self.h

    def leaves(self):
        return self.obs.copy(), self.mask.copy(), self.status.copy()

    def advance(self, priors, values):
        priors, values = np.ascontiguousarray(priors, F), np.ascontiguousarray(values, F)
        assert priors.shape == (self.n, self.n_act) and values.shape == (self.n,)
        return self.lib.pgx_guided_advance(ctypes.c_void_p(self.h), _ptr(priors), _ptr(values), _ptr(self.obs),
                                           _ptr(self.mask), _ptr(self.status))

    def result(self):
        visits, values = np.full((self.n, self.n_act), -7, np.int32), np.full((self.n, self.n_act), -7, F)
        action, nodes = np.full(self.n, -7, np.int32), np.zeros(self.n, np.int32)
        self.lib.pgx_guided_result(ctypes.c_void_p(self.h), _ptr(visits), _ptr(values), _ptr(action), _ptr(nodes))
        return visits, values, action, nodes

    def close(self):
        self.lib.pgx_guided_end(ctypes.c_void_p(self.h))
        self.h = None


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def both(libs, game_, pos, simulations, c_puct, evaluate=stand_in, spoil=None):
    """The numpy restatement and the harness from `pos`, fed the same evaluator, compared after every call: the leaves,
    the visit sum and the result, bit for bit.  `spoil(t, priors, values, status)`: changes the rows in place before
    they are fed.  Returns (the harness's final result, the statuses seen)."""
    tree = GuidedTree(pos, pos.done, game_.expand, simulations, c_puct)
    host = HostSession(libs, game_.tid, [pos], simulations, c_puct)
    seen = []
    for t in range(simulations + 1):
        obs, mask, status = host.leaves()
        want = tree.leaf()
        assert status[0] == want[2], (game_.tid, t)
        assert np.array_equal(obs[0].astype(bool), want[0]) and np.array_equal(mask[0].astype(bool), want[1]), t
        assert set(np.unique(obs)) <= {0, 1} and set(np.unique(mask)) <= {0, 1}
        if status[0] != 0:
            assert not obs.any() and not mask.any()
        seen.append(int(status[0]))
        priors, values = evaluate(obs, mask)
        if spoil is not None:
            spoil(t, priors, values, status)
        assert host.advance(priors, values) == 0
        tree.advance(priors[0], values[0])
        got, ref = host.result(), tree.result()
        assert np.array_equal(got[0][0], ref[0]), (game_.tid, t, got[0][0], ref[0])
        assert np.array_equal(bits(got[1][0]), bits(ref[1])), (game_.tid, t, got[1][0], ref[1])
        assert got[2][0] == ref[2] and got[3][0] == ref[3]
        assert got[0].sum() == (0 if pos.done else t)  # after advance t the visits sum to t
        assert got[3][0] <= simulations + 1
    assert host.status[0] == 2 and not host.obs.any() and not host.mask.any()
    assert host.advance(priors, values) == -4  # a call number above S
    out = host.result()
    host.close()
    assert (out[0][0][~pos.mask] == 0).all() and (out[1][0][~pos.mask] == 0).all()
    return out, seen


def mid_row(g, column):
    """A fixture row a few plies into a game at which the column's env is not over."""
    return next(t for t in range(4, len(g["done"])) if not g["done"][t, column] and g["elapsed_step"][t, column] >= 3)


@pytest.mark.parametrize("c_puct", [1.25, 0.0])
@pytest.mark.parametrize("mid", [False, True])
@pytest.mark.parametrize("tid", GAMES)
def test_host_session_equals_the_numpy_restatement(libs, tid, mid, c_puct):
    game_ = Replayed(libs, tid, column=2 if mid else 1)
    t0 = mid_row(game_.g, 2) if mid else 0
    pos = game_.fixture_row(t0)
    assert not pos.done
    # the root's emitted rows are the fixture's own rows for the mover
    g, col = game_.g, game_.column
    assert np.array_equal(pos.obs, g["obs"][t0, col, pos.mover].astype(bool))
    assert np.array_equal(pos.mask, g["info:legal_action_mask"][t0, col].astype(bool))
    (visits, values, action, nodes), seen = both(libs, game_, pos, S, c_puct)
    assert action[0] >= 0 and pos.mask[action[0]] and visits.sum() == S
    assert nodes[0] == len(game_.expanded) + 1
    if c_puct > 0 and pos.mask.sum() > 4:
        assert (visits[0] > 0).sum() > 1  # exploration spreads the visits
    if c_puct == 0 and not mid:
        assert 0 in seen


def test_emitted_rows_along_a_fixture_game(libs):
    """begin at every row of a fixture game: obs and mask are the fixture's rows of the seat to move, zeros when over."""
    for tid in GAMES:
        game_ = Replayed(libs, tid, column=0)
        g = game_.g
        rows = [t for t in range(0, 12) if g["elapsed_step"][t, 0] == t]  # the first game of the column
        poss = [game_.fixture_row(t) for t in rows]
        host = HostSession(libs, tid, poss, 4, 1.25)
        obs, mask, status = host.leaves()
        host.close()
        for i, t in enumerate(rows):
            if g["done"][t, 0]:
                assert status[i] == 2 and not obs[i].any() and not mask[i].any()
            else:
                mover = int(g["info:current_player"][t, 0])
                assert status[i] == 0
                assert np.array_equal(obs[i], g["obs"][t, 0, mover]), (tid, t)
                assert np.array_equal(mask[i], g["info:legal_action_mask"][t, 0]), (tid, t)


def test_a_root_that_is_over_reports_zeros(libs):
    game_ = Replayed(libs, "TicTacToe-v1", column=0)
    t0 = int(np.flatnonzero(game_.g["done"][:, 0])[0])
    pos = game_.fixture_row(t0)
    assert pos.done
    (visits, values, action, nodes), seen = both(libs, game_, pos, S, 1.25)
    assert action[0] == -1 and not visits.any() and not values.any() and set(seen) == {2}


def test_terminal_leaves_are_valued_by_the_game_and_revisited(libs):
    """TicTacToe with three empty cells: at most 1 + 3 + 6 + 6 nodes, so most of 64 simulations end in a node whose
    game is over -- new (expanded into) or old (descended into again): status 1, and whatever the caller's row says
    there is ignored."""
    game_ = Replayed(libs, "TicTacToe-v1", column=0)
    pos, _ = game_.at([0, 1, 2, 4, 3, 5])
    assert not pos.done and pos.mask.sum() == 3
    plain, seen = both(libs, game_, pos, 64, 1.25)
    assert plain[3][0] <= 16 and seen.count(1) > 64 - 16  # terminal nodes are revisited
    assert seen.count(1) > plain[3][0]

    def spoil(t, priors, values, status):
        if status[0] == 1:
            priors[:] = 1e30 * (t + 1)
            values[:] = -1.0 if t % 2 else 1.0

    game2 = Replayed(libs, "TicTacToe-v1", column=0)
    spoiled, seen2 = both(libs, game2, pos, 64, 1.25, spoil=spoil)
    assert seen2 == seen
    for a, b in zip(plain, spoiled):
        assert np.array_equal(a, b)


def test_clean_and_cleanv(libs):
    """NaN, inf and a negative prior count as 0; NaN, inf and 2 as values count as 0: the search equals the one fed
    zeros in their place (and the restatement, which cleans on its own)."""
    junk = [np.nan, np.inf, -np.inf, -0.25]
    for tid in ("ConnectFour-v1", "Othello-v1"):
        pos = Replayed(libs, tid, column=1).fixture_row(0)

        def dirty(t, priors, values, status):
            legal = np.flatnonzero(priors[0] > 0)
            if len(legal) == 0:
                return
            priors[0, legal[t % len(legal)]] = junk[t % 4]
            if t % 3 == 0:
                values[0] = [2.0, np.nan, -np.inf, 1.0000001][(t // 3) % 4]

        def zeroed(t, priors, values, status):
            dirty(t, priors, values, status)
            priors[~(np.isfinite(priors) & (priors >= 0))] = 0.0
            values[~((values >= -1) & (values <= 1))] = 0.0

        a, _ = both(libs, Replayed(libs, tid, column=1), pos, S, 1.25, spoil=dirty)
        b, _ = both(libs, Replayed(libs, tid, column=1), pos, S, 1.25, spoil=zeroed)
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=False)
        assert np.isfinite(a[1]).all()
        c, _ = both(libs, Replayed(libs, tid, column=1), pos, S, 1.25)
        assert not np.array_equal(bits(a[1]), bits(c[1]))  # the junk was in rows that count


def test_hex_swap_and_second_slots(libs):
    """Hex one stone in: 120 cells and the swap (action 121) are legal; with uniform priors, zero values and S > 121
    every one of them is tried once: the second action of a lane is scored, picked, expanded and backed up."""
    game_ = Replayed(libs, "Hex-v1", column=0)
    pos, _ = game_.at([60])
    assert pos.mask[121] and pos.mask.sum() == 121

    def flat(obs, mask):
        return (mask > 0).astype(F) / F(128.0), np.zeros(len(mask), F)

    (visits, values, action, nodes), _ = both(libs, game_, pos, 124, 1.25, evaluate=flat)
    assert visits[0][121] >= 1 and 121 in game_.expanded and (visits[0][pos.mask] >= 1).all()


def test_othello_forced_pass(libs):
    """The pass (action 64) is lane 0's second slot; here it is the only legal move of the root."""
    game_ = Replayed(libs, "Othello-v1", column=0)
    rng = np.random.default_rng(5)
    found = None
    for _ in range(400):
        seq = []
        pos, _ = game_.at(seq)
        while not pos.done and found is None:
            if pos.mask[64]:
                assert pos.mask.sum() == 1
                found = pos
                break
            seq.append(int(rng.choice(np.flatnonzero(pos.mask))))
            pos, _ = game_.at(seq)
        if found is not None:
            break
    assert found is not None, "no forced pass found"
    (visits, values, action, nodes), _ = both(libs, game_, found, S, 1.25)
    assert visits[0][64] == S and action[0] == 64 and nodes[0] > 2


def test_a_win_in_one_is_found(libs):
    """TicTacToe, the mover has two in a row: uniform priors and zero values -- only the game's own outcomes count."""
    game_ = Replayed(libs, "TicTacToe-v1", column=0)
    pos, _ = game_.at([0, 3, 1, 4])
    assert not pos.done and pos.mask[2] and pos.mask.sum() == 5

    def flat(obs, mask):
        return (mask > 0).astype(F) / F(8.0), np.zeros(len(mask), F)

    (visits, values, action, nodes), seen = both(libs, game_, pos, S, 1.25, evaluate=flat)
    assert action[0] == 2 and visits[0][2] > S // 2 and values[0][2] == visits[0][2]  # every visit of it is a win
    assert 1 in seen


def test_flipping_every_value_flips_the_preference(libs):
    """TicTacToe with cells 6 and 8 empty.  The evaluator calls the leaf behind move 6 good for the seat that moves
    there (so bad for the root's mover) and the one behind move 8 bad, every other leaf 0: the search prefers 8.  With
    every value negated it prefers 6."""
    game_ = Replayed(libs, "TicTacToe-v1", column=0)
    pos, _ = game_.at([0, 1, 2, 4, 3, 5, 7])
    assert not pos.done and np.flatnonzero(pos.mask).tolist() == [6, 8]

    def evaluator(sign):
        def evaluate(obs, mask):
            m = mask[0].astype(bool)
            v = 0.0
            if m.sum() == 1:
                v = 0.5 if m[8] else -0.5  # only 8 left: the leaf behind move 6
            return (mask > 0).astype(F) / F(2.0), np.array([sign * v], F)
        return evaluate

    (v1, _, a1, _), _ = both(libs, game_, pos, 3, 0.1, evaluate=evaluator(1.0))
    (v2, _, a2, _), _ = both(libs, Replayed(libs, "TicTacToe-v1", column=0), pos, 3, 0.1, evaluate=evaluator(-1.0))
    assert a1[0] == 8 and v1[0][8] > v1[0][6]
    assert a2[0] == 6 and v2[0][6] > v2[0][8]


def test_several_roots_in_one_session(libs):
    """Rows are independent: a session over three roots, one of them over, equals three sessions of one."""
    game_ = Replayed(libs, "ConnectFour-v1", column=2)
    g = game_.g
    over = int(np.flatnonzero(g["done"][:, 2])[0])
    poss = [game_.fixture_row(0), game_.fixture_row(over), game_.fixture_row(mid_row(g, 2))]
    assert [p.done for p in poss] == [False, True, False]
    many = HostSession(libs, game_.tid, poss, 8, 1.25)
    ones = [HostSession(libs, game_.tid, [p], 8, 1.25) for p in poss]
    for t in range(9):
        obs, mask, status = many.leaves()
        for i, one in enumerate(ones):
            for a, b in zip((obs, mask, status), one.leaves()):
                assert np.array_equal(a[i:i + 1], b)
        priors, values = stand_in(obs, mask)
        assert many.advance(priors, values) == 0
        for i, one in enumerate(ones):
            assert one.advance(priors[i:i + 1], values[i:i + 1]) == 0
    for i, one in enumerate(ones):
        for a, b in zip(many.result(), one.result()):
            assert np.array_equal(a[i:i + 1], b)
        one.close()
    many.close()


def test_node_layout(libs):
    """80 bytes of State and term0, then four 4-byte arrays of A rounded up to whole 16-byte words."""
    for name, n_act in ACTIONS.items():
        assert libs[1].pgx_guided_node_bytes(CODE[name]) == 80 + 4 * 4 * ((n_act + 3) // 4 * 4)


def test_stand_in_evaluator():
    rng = np.random.default_rng(0)
    obs, mask = rng.random((5, 8, 8, 2)) < 0.3, rng.random((5, 65)) < 0.4
    mask[4] = False
    p, v = stand_in(obs, mask)
    assert p.dtype == F and v.dtype == F and p.shape == (5, 65) and v.shape == (5,)
    assert (p[~mask] == 0).all() and (p[mask] > 0).all() and np.allclose(p[:4].sum(1), 1, atol=1e-5)
    assert not p[4].any() and (np.abs(v) <= 1).all() and len(np.unique(v[:4])) == 4
    q, w = stand_in(obs.copy(), mask.copy())
    assert np.array_equal(p, q) and np.array_equal(v, w)


# ---- argument checks ----------------------------------------------------------------------------------------------
BAD = [dict(simulations=0), dict(simulations=4097), dict(c_puct=-0.5), dict(c_puct=float("nan")),
       dict(c_puct=float("inf")), dict(c_puct=1e39)]


def test_check_guided():
    from envpool_amd.core import native

    ids = native.check_guided([[3, 1], [2, 2]], 64, 1.25)
    assert ids.dtype == np.int32 and ids.tolist() == [3, 1, 2, 2]  # ids may repeat
    native.check_guided([0], 4096, 0.0)
    native.check_guided([0], 1, 3.0)
    base = dict(simulations=64, c_puct=1.25)
    for kw in BAD:
        with pytest.raises(ValueError, match="guided_begin"):
            native.check_guided([0], **{**base, **kw})
    with pytest.raises(ValueError, match="empty"):
        native.check_guided(np.zeros(0, np.int32), **base)
    p, v = native.check_guided_rows([[0.5, 0.5, 0.0]] * 2, [1, -1], 2, 3)
    assert p.dtype == np.float32 and v.dtype == np.float32 and p.flags.c_contiguous
    for priors, values in (([[0.5, 0.5, 0.0]], [0.0]), ([[0.5, 0.5]] * 2, [0.0, 0.0]), ([[0.5, 0.5, 0.0]] * 2, [0.0]),
                           ([[0.5, np.nan, 0.0]] * 2, [0.0, 0.0]), ([[0.5, np.inf, 0.0]] * 2, [0.0, 0.0]),
                           ([[0.5, -0.1, 0.0]] * 2, [0.0, 0.0]), ([[0.5, 0.5, 0.0]] * 2, [0.0, 2.0]),
                           ([[0.5, 0.5, 0.0]] * 2, [np.nan, 0.0])):
        with pytest.raises(ValueError, match="guided_advance"):
            native.check_guided_rows(priors, values, 2, 3)


class _Recorder:
    """A pool that records the guided calls it gets."""

    def __init__(self):
        self.calls = []

    def guided_begin(self, env_ids, simulations, c_puct):
        self.calls.append(("begin", np.asarray(env_ids).tolist(), simulations, c_puct))
        self.k = len(env_ids)
        return self._leaves()

    def _leaves(self):
        return np.zeros((self.k, 8, 8, 2), bool), np.zeros((self.k, 65), bool), np.zeros(self.k, np.uint8)

    def guided_advance(self, priors, values):
        self.calls.append(("advance", np.asarray(priors).shape, np.asarray(values).shape))
        return self._leaves()

    def guided_result(self):
        self.calls.append(("result",))
        return np.zeros((self.k, 65), np.int32), np.zeros((self.k, 65), np.float32), np.zeros(self.k, np.int32)

    def guided_end(self):
        self.calls.append(("end",))


def test_wrapper_checks_come_before_the_native_call():
    from envpool_amd.pgx import OthelloGymnasiumEnvPool

    env = object.__new__(OthelloGymnasiumEnvPool)
    env._pool = _Recorder()
    ids = np.array([2, 0, 1], np.int32)
    for kw in BAD:
        with pytest.raises(ValueError, match="guided_begin"):
            env.guided_search(ids, **kw)
    with pytest.raises(ValueError, match="empty"):
        env.guided_search(np.zeros(0, np.int32))
    assert env._pool.calls == []
    gs = env.guided_search(ids, simulations=3, c_puct=0.5)
    assert env._pool.calls == [("begin", [2, 0, 1], 3, 0.5)]
    assert [x.shape for x in gs.leaves] == [(3, 8, 8, 2), (3, 65), (3,)]
    seen = []

    def evaluate(obs, mask, status):
        seen.append((obs.shape, mask.shape, status.shape))
        return np.zeros((3, 65), np.float32), np.zeros(3, np.float32)

    out = gs.run(evaluate)
    assert out._fields == ("visits", "values", "action") and len(seen) == 4  # S + 1 evaluations
    assert [c[0] for c in env._pool.calls] == ["begin"] + ["advance"] * 4 + ["result", "end"]
    with pytest.raises(ValueError, match="closed"):
        gs.advance(np.zeros((3, 65), np.float32), np.zeros(3, np.float32))
    gs.close()  # (twice: nothing)
    assert env._pool.calls[-1] == ("end",) and len(env._pool.calls) == 7
    gs = env.guided_search(ids, simulations=1)
    gs.advance(*evaluate(*gs.leaves))
    gs.advance(*evaluate(*gs.leaves))
    with pytest.raises(ValueError, match="above simulations"):
        gs.advance(*evaluate(*gs.leaves))
