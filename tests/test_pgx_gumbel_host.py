"""PGX Gumbel search, CPU side: the stepwise search of envpool_amd/csrc/pgx_gumbel.hip.h built for the host by g++ (a
harness that walks a wave's lanes as loops) against the contract restated in numpy float32 (pgx_gumbel_util.py), which
keeps the tree in Python, takes every position, observation and expansion step from the reference-pinned `pgx_replay`
of the PGX host harness and shares no code with the header; the header's exponential and its walk of the table of
considered visits; what the search must do whatever its arithmetic (the visit counts of sequential halving, minimax-
optimal moves from exact values); and the argument checks of the Python wrappers, which come before any native call."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from pgx_gumbel_util import (GumbelTree, exp_, gumbel_noise, sequence_of_considered_visits, stand_in_logits,
                             visit_multiset, wild_logits)
from pgx_util import ACTIONS, CODE, game
from test_pgx_guided_host import Replayed, mid_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMES = ["TicTacToe-v1", "ConnectFour-v1", "Hex-v1", "Othello-v1"]
F = np.float32


def _build(tmp, source, name):
    out = str(tmp / name)
    # no fast-math, no contraction: every float operation rounds on its own
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "cpu_harness", source), "-o", out], check=True)
    return ctypes.CDLL(out)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pgx_gumbel")
    gumbel = _build(tmp, "pgx_gumbel_host.cpp", "libpgxgumbelhost.so")
    gumbel.pgx_gumbel_begin.restype = ctypes.c_void_p
    gumbel.pgx_gumbel_result.restype = None
    gumbel.pgx_gumbel_end.restype = None
    gumbel.pgx_gumbel_exp.restype = None
    return _build(tmp, "pgx_host.cpp", "libpgxhost.so"), gumbel


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


class HostSession:
    """The harness's session over the roots `poss` (Pos with key = (seq, hidden words))."""

    def __init__(self, libs, tid, poss, simulations, considered, gumbel, c_visit=50.0, c_scale=0.1):
        self.lib, self.n, self.n_act = libs[1], len(poss), ACTIONS[game(tid)]
        hid = np.ascontiguousarray(np.stack([p.key[1] for p in poss]), np.int32)
        done = np.array([p.done for p in poss], np.uint8)
        gumbel = np.ascontiguousarray(gumbel, F)
        assert gumbel.shape == (self.n, self.n_act)
        self.obs = np.full((self.n,) + poss[0].obs.shape, 7, np.uint8)
        self.mask = np.full((self.n, self.n_act), 7, np.uint8)
        self.status = np.full(self.n, 7, np.uint8)
        rc = ctypes.c_int(-9)
        self.h = self.lib.pgx_gumbel_begin(CODE[game(tid)], self.n, _ptr(hid), _ptr(done), simulations, considered,
                                           ctypes.c_float(c_visit), ctypes.c_float(c_scale), _ptr(gumbel),
                                           _ptr(self.obs), _ptr(self.mask), _ptr(self.status), ctypes.byref(rc))
        assert rc.value == 0 and self.h

    def leaves(self):
        return self.obs.copy(), self.mask.copy(), self.status.copy()

    def advance(self, logits, values):
        logits, values = np.ascontiguousarray(logits, F), np.ascontiguousarray(values, F)
        assert logits.shape == (self.n, self.n_act) and values.shape == (self.n,)
        return self.lib.pgx_gumbel_advance(ctypes.c_void_p(self.h), _ptr(logits), _ptr(values), _ptr(self.obs),
                                           _ptr(self.mask), _ptr(self.status))

    def result(self):
        visits, values = np.full((self.n, self.n_act), -7, np.int32), np.full((self.n, self.n_act), -7, F)
        action, nodes = np.full(self.n, -7, np.int32), np.zeros(self.n, np.int32)
        weights = np.full((self.n, self.n_act), -7, F)
        self.lib.pgx_gumbel_result(ctypes.c_void_p(self.h), _ptr(visits), _ptr(values), _ptr(action), _ptr(weights),
                                   _ptr(nodes))
        return visits, values, action, weights, nodes

    def close(self):
        self.lib.pgx_gumbel_end(ctypes.c_void_p(self.h))
        self.h = None


def both(libs, game_, pos, simulations, considered, gumbel, evaluate=stand_in_logits, **consts):
    """The numpy restatement and the harness from `pos`, fed the same evaluator, compared after every call: the leaves
    and the result, bit for bit.  Returns (the harness's final result, the statuses seen)."""
    tree = GumbelTree(pos, pos.done, game_.expand, simulations, considered, gumbel, **consts)
    host = HostSession(libs, game_.tid, [pos], simulations, considered, gumbel[None, :], **consts)
    where = (game_.tid, simulations, considered)
    seen = []
    for t in range(simulations + 1):
        obs, mask, status = host.leaves()
        want = tree.leaf()
        assert status[0] == want[2], (where, t)
        assert np.array_equal(obs[0].astype(bool), want[0]) and np.array_equal(mask[0].astype(bool), want[1]), (where, t)
        if status[0] != 0:
            assert not obs.any() and not mask.any()
        seen.append(int(status[0]))
        logits, values = evaluate(obs, mask)
        assert host.advance(logits, values) == 0
        tree.advance(logits[0], values[0])
        got, ref = host.result(), tree.result()
        assert np.array_equal(got[0][0], ref[0]), (where, t, got[0][0], ref[0])
        assert np.array_equal(bits(got[1][0]), bits(ref[1])), (where, t, got[1][0], ref[1])
        assert got[2][0] == ref[2], (where, t, got[2][0], ref[2])
        assert np.array_equal(bits(got[3][0]), bits(ref[3])), (where, t, got[3][0], ref[3])
        assert got[4][0] == ref[4]
        assert got[0].sum() == (0 if pos.done else t)  # after advance t the visits sum to t
    assert host.status[0] == 2 and not host.obs.any() and not host.mask.any()
    assert host.advance(logits, values) == -4  # a call number above S
    out = host.result()
    host.close()
    check_structure(pos, out, simulations, considered, gumbel)
    return out, seen


def check_structure(pos, out, simulations, considered, gumbel):
    """What a finished search of a root must show, whatever its arithmetic."""
    visits, values, action, weights, _ = (x[0] for x in out)
    if pos.done:
        assert action == -1 and not visits.any() and not values.any() and not weights.any()
        return
    mask = pos.mask
    assert visits.sum() == simulations and (visits[~mask] == 0).all() and (values[~mask] == 0).all()
    assert (weights[~mask] == 0).all() and (weights[mask] > 0).all() and abs(float(weights.sum(dtype=np.float64)) - 1) < 1e-6
    assert mask[action] and visits[action] == visits.max()
    m_eff = min(considered, int(mask.sum()))
    assert sorted(visits[visits > 0].tolist()) == [c for c in visit_multiset(m_eff, simulations) if c > 0]
    return m_eff


def seeded(tid, seed=7):
    return gumbel_noise(seed, 1, ACTIONS[game(tid)])[0]


# ---- the header's integer walk and its exponential ------------------------------------------------------------------
def test_considered_visit_walk_equals_the_sequence(libs):
    walk = libs[1].pgx_gumbel_considered_visit
    for m in range(1, max(ACTIONS.values()) + 1):
        for s in (1, 2, 7, 16, 33, 64):
            assert [walk(m, s, t) for t in range(s)] == sequence_of_considered_visits(m, s), (m, s)


def test_exp_bit_for_bit_and_its_error(libs):
    grid = np.concatenate([np.array([0.0, -0.0, -87.0, -87.5, -100.0, -1e30, -np.inf, 1e-3, 5.0, -1e-30, -1e-45], F),
                           np.linspace(-87.0, 0.0, 200001).astype(F),
                           -np.exp(np.linspace(np.log(1e-8), np.log(87.0), 20001)).astype(F)])
    out = np.empty_like(grid)
    libs[1].pgx_gumbel_exp(_ptr(grid), len(grid), _ptr(out))
    assert np.array_equal(out.view(np.uint32), exp_(grid).view(np.uint32))
    assert out[0] == 1 and out[1] == 1 and out[2] == out[3] == out[4] == out[5] == out[6] and out[7] == 1
    inside = (grid >= -87) & (grid <= 0)
    exact = np.exp(grid[inside].astype(np.float64))
    assert np.max(np.abs(out[inside] / exact - 1)) < 3e-7  # (DESIGN.md states the measured maximum)
    order = np.argsort(grid[inside], kind="stable")
    assert (np.diff(out[inside][order]) >= 0).all() and out.min() > np.finfo(F).tiny


# ---- the harness against the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("simulations", [1, 7, 16])
@pytest.mark.parametrize("tid", GAMES)
def test_host_session_equals_the_numpy_restatement(libs, tid, simulations):
    """Every m of {1, 2, 4, 16, A}; a mid-game fixture row with the stand-in evaluator and seeded noise, and the
    start of a game with the large-magnitude, tied logits and no noise."""
    n_act = ACTIONS[game(tid)]
    mid = Replayed(libs, tid, column=2)
    mid_pos = mid.fixture_row(mid_row(mid.g, 2))
    start = Replayed(libs, tid, column=1)
    start_pos = start.fixture_row(0)
    assert not mid_pos.done and not start_pos.done
    for m in sorted({min(m, n_act) for m in (1, 2, 4, 16, n_act)}):
        (visits, _, action, weights, nodes), seen = both(libs, mid, mid_pos, simulations, m, seeded(tid))
        assert 0 in seen and nodes[0] <= simulations + 1
        both(libs, start, start_pos, simulations, m, np.zeros(n_act, F), evaluate=wild_logits)
    if tid == "Hex-v1":
        assert mid_pos.mask[64:].any()  # the second slot of a lane is live


def test_the_top_m_actions_by_gumbel_plus_logits_get_the_visits(libs):
    for tid in ("ConnectFour-v1", "Othello-v1", "Hex-v1"):
        game_ = Replayed(libs, tid, column=2)
        pos = game_.fixture_row(mid_row(game_.g, 2))
        for gumbel in (np.zeros(ACTIONS[game(tid)], F), seeded(tid, 3)):
            for m in (2, 4):
                out, _ = both(libs, game_, pos, 16, m, gumbel)
                logits, _ = stand_in_logits(pos.obs[None], pos.mask[None])
                key = np.where(pos.mask, (gumbel + logits[0]).astype(np.float64), -np.inf)
                top = set(np.argsort(-key, kind="stable")[:min(m, int(pos.mask.sum()))].tolist())
                assert set(np.flatnonzero(out[0][0]).tolist()) == top, (tid, m)


def test_consts_and_noise_are_cleaned(libs):
    """Other c_visit / c_scale, a zero scale, and noise that is not finite (counts as 0)."""
    game_ = Replayed(libs, "ConnectFour-v1", column=1)
    pos = game_.fixture_row(0)
    dirty = seeded("ConnectFour-v1")
    dirty[[1, 3, 5]] = [np.nan, np.inf, -np.inf]
    zeroed = dirty.copy()
    zeroed[[1, 3, 5]] = 0
    a, _ = both(libs, game_, pos, 16, 4, dirty, c_visit=10.0, c_scale=1.0)
    b, _ = both(libs, Replayed(libs, "ConnectFour-v1", column=1), pos, 16, 4, zeroed, c_visit=10.0, c_scale=1.0)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    both(libs, game_, pos, 7, 7, zeroed, c_visit=0.0, c_scale=0.0)
    both(libs, game_, pos, 7, 7, zeroed, c_visit=3e38, c_scale=3e38, evaluate=wild_logits)  # the scale's cap


def test_a_root_one_ply_from_the_end_and_a_root_that_is_over(libs):
    """TicTacToe with three empty cells: most simulations end in a finished game, status 1."""
    game_ = Replayed(libs, "TicTacToe-v1", column=0)
    pos, _ = game_.at([0, 1, 2, 4, 3, 5])
    assert not pos.done and pos.mask.sum() == 3
    for m in (1, 2, 9):
        out, seen = both(libs, game_, pos, 16, m, seeded("TicTacToe-v1"))
        assert 1 in seen
    over = game_.fixture_row(int(np.flatnonzero(game_.g["done"][:, 0])[0]))
    assert over.done
    out, seen = both(libs, game_, over, 7, 4, seeded("TicTacToe-v1"))
    assert out[2][0] == -1 and set(seen) == {2}


def test_othello_forced_pass(libs):
    """The pass (action 64) is lane 0's second slot, and the only action there; here it is the root's only move."""
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
    for m in (1, 16):
        out, _ = both(libs, game_, found, 7, m, seeded("Othello-v1"))
        assert out[0][0][64] == 7 and out[2][0] == 64 and out[3][0][64] == 1


def test_several_roots_in_one_session(libs):
    """Rows are independent: a session over three roots, one of them over, equals three sessions of one."""
    game_ = Replayed(libs, "ConnectFour-v1", column=2)
    g = game_.g
    over = int(np.flatnonzero(g["done"][:, 2])[0])
    poss = [game_.fixture_row(0), game_.fixture_row(over), game_.fixture_row(mid_row(g, 2))]
    assert [p.done for p in poss] == [False, True, False]
    noise = gumbel_noise(1, 3, 7)
    many = HostSession(libs, game_.tid, poss, 8, 4, noise)
    ones = [HostSession(libs, game_.tid, [p], 8, 4, noise[i:i + 1]) for i, p in enumerate(poss)]
    for t in range(9):
        obs, mask, status = many.leaves()
        for i, one in enumerate(ones):
            for a, b in zip((obs, mask, status), one.leaves()):
                assert np.array_equal(a[i:i + 1], b)
        logits, values = stand_in_logits(obs, mask)
        assert many.advance(logits, values) == 0
        for i, one in enumerate(ones):
            assert one.advance(logits[i:i + 1], values[i:i + 1]) == 0
    for i, one in enumerate(ones):
        for a, b in zip(many.result(), one.result()):
            assert np.array_equal(a[i:i + 1], b)
        one.close()
    many.close()


def test_node_layout(libs):
    """80 bytes of State, term0 and raw, then five 4-byte arrays of A rounded up to whole 16-byte words."""
    for name, n_act in ACTIONS.items():
        assert libs[1].pgx_gumbel_node_bytes(CODE[name]) == 80 + 5 * 4 * ((n_act + 3) // 4 * 4)


# ---- semantics, independent of the restatement ----------------------------------------------------------------------
LINES = [(0, 1, 2), (3, 4, 5), (6, 7, 8), (0, 3, 6), (1, 4, 7), (2, 5, 8), (0, 4, 8), (2, 4, 6)]


def minimax(mine, theirs, memo):
    """The exact value of a TicTacToe position for the seat to move: `mine`, `theirs` are the cell sets."""
    key = (mine, theirs)
    if key not in memo:
        if any(all(c in theirs for c in line) for line in LINES):
            memo[key] = -1
        elif len(mine) + len(theirs) == 9:
            memo[key] = 0
        else:
            memo[key] = max(-minimax(theirs, mine | {c}, memo) for c in range(9) if c not in mine and c not in theirs)
    return memo[key]


def tictactoe_cells(obs):
    """(the mover's cells, the other seat's) of an emitted obs row [3, 3, 2]: plane 0 is the seat to move."""
    flat = np.asarray(obs, bool).reshape(9, 2)
    return frozenset(np.flatnonzero(flat[:, 0]).tolist()), frozenset(np.flatnonzero(flat[:, 1]).tolist())


def exact_evaluator(memo):
    def evaluate(obs, mask):
        values = np.array([minimax(*tictactoe_cells(o), memo) if m.any() else 0 for o, m in zip(obs, mask)], F)
        return np.zeros(mask.shape, F), values
    return evaluate


def optimal_moves(mine, theirs, memo):
    best = minimax(mine, theirs, memo)
    return {c for c in range(9) if c not in mine and c not in theirs and -minimax(theirs, mine | {c}, memo) == best}


def two_ply_roots(game_):
    """Every TicTacToe position two plies after the reset: 7 legal actions, none of them ends the game."""
    roots = {}
    for a in range(9):
        for b in range(9):
            if a != b:
                pos, _ = game_.at([a, b])
                assert not pos.done and pos.mask.sum() == 7
                roots[pos.key[1].tobytes()] = pos
    assert len(roots) >= 30
    return list(roots.values())


def test_exact_values_give_minimax_optimal_moves(libs):
    """S = 7, m = 16, no noise, zero logits, and the evaluator returns the exact minimax value of every leaf for the
    seat to move: each of the 7 root actions is visited once, its q is exact and sigma is monotone in it, so the
    recommended action and the arg-max of the improved policy are minimax-optimal.  A sign or seat error anywhere
    between the emitted observation and the root's q fails this, whatever the restatement says."""
    game_ = Replayed(libs, "TicTacToe-v1", column=0)
    roots = two_ply_roots(game_)
    memo = {}
    # the obs planes: plane 0 holds the mover's cells
    first, _ = game_.at([1])
    mine, theirs = tictactoe_cells(first.obs)
    assert mine == frozenset() and theirs == frozenset({1})
    host = HostSession(libs, game_.tid, roots, 7, 16, np.zeros((len(roots), 9), F))
    evaluate = exact_evaluator(memo)
    for _ in range(8):
        obs, mask, status = host.leaves()
        assert host.advance(*evaluate(obs, mask)) == 0
    visits, values, action, weights, _ = host.result()
    host.close()
    varied = set()
    for i, pos in enumerate(roots):
        assert np.array_equal(visits[i], pos.mask.astype(np.int32))  # every root action exactly once
        best = optimal_moves(*tictactoe_cells(pos.obs), memo)
        varied.add(len(best))
        assert int(action[i]) in best, (i, action[i], best)
        assert int(np.argmax(weights[i])) in best
        mine, theirs = tictactoe_cells(pos.obs)
        for c in np.flatnonzero(pos.mask):  # each q is the exact value of the move
            assert values[i][c] == -minimax(theirs, mine | {int(c)}, memo)
    assert len(varied) > 1  # some roots have few optimal moves, some many


# ---- argument checks ------------------------------------------------------------------------------------------------
BAD = [dict(simulations=0), dict(simulations=4097), dict(max_considered=0), dict(max_considered=-3),
       dict(c_visit=-0.5), dict(c_visit=float("nan")), dict(c_scale=float("inf")), dict(c_scale=-1.0),
       dict(c_scale=1e39)]


def test_check_gumbel():
    from envpool_amd.core import native

    base = dict(simulations=32, max_considered=16, c_visit=50.0, c_scale=0.1)
    ids = native.check_gumbel([[3, 1], [2, 2]], **base)
    assert ids.dtype == np.int32 and ids.tolist() == [3, 1, 2, 2]  # ids may repeat
    native.check_gumbel([0], 4096, 1, 0.0, 0.0)
    native.check_gumbel([0], 1, 1000, 50.0, 0.1)  # above the game's actions: all of them
    for kw in BAD:
        with pytest.raises(ValueError, match="gumbel_begin"):
            native.check_gumbel([0], **{**base, **kw})
    with pytest.raises(ValueError, match="empty"):
        native.check_gumbel(np.zeros(0, np.int32), **base)
    g = native.check_gumbel_noise([[0.5, -0.5, 0.0]] * 2, 2, 3)
    assert g.dtype == np.float32 and g.flags.c_contiguous
    for noise in ([[0.5, 0.5, 0.0]], [[0.5, 0.5]] * 2, [0.5, 0.5, 0.0], [[0.5, np.nan, 0.0]] * 2,
                  [[0.5, np.inf, 0.0]] * 2):
        with pytest.raises(ValueError, match="gumbel_begin"):
            native.check_gumbel_noise(noise, 2, 3)
    p, v = native.check_gumbel_rows([[0.5, -7.5, 0.0]] * 2, [1, -1], 2, 3)  # logits may be negative
    assert p.dtype == np.float32 and v.dtype == np.float32 and p.flags.c_contiguous and p[0, 1] == -7.5
    for logits, values in (([[0.5, 0.5, 0.0]], [0.0]), ([[0.5, 0.5]] * 2, [0.0, 0.0]), ([[0.5, 0.5, 0.0]] * 2, [0.0]),
                           ([[0.5, np.nan, 0.0]] * 2, [0.0, 0.0]), ([[0.5, np.inf, 0.0]] * 2, [0.0, 0.0]),
                           ([[0.5, -np.inf, 0.0]] * 2, [0.0, 0.0]), ([[0.5, 2e30, 0.0]] * 2, [0.0, 0.0]),
                           ([[0.5, 0.5, 0.0]] * 2, [0.0, 2.0]), ([[0.5, 0.5, 0.0]] * 2, [np.nan, 0.0])):
        with pytest.raises(ValueError, match="gumbel_advance"):
            native.check_gumbel_rows(logits, values, 2, 3)


class _Recorder:
    """A pool that records the search calls it gets."""

    def __init__(self):
        self.calls = []

    def gumbel_actions(self):
        return 65

    def _leaves(self):
        return np.zeros((self.k, 8, 8, 2), bool), np.zeros((self.k, 65), bool), np.zeros(self.k, np.uint8)

    def gumbel_begin(self, gumbel, env_ids, simulations, max_considered, c_visit, c_scale):
        self.calls.append(("begin", np.asarray(env_ids).tolist(), simulations, max_considered, c_visit, c_scale))
        self.k, self.gumbel = len(env_ids), gumbel
        return self._leaves()

    def gumbel_advance(self, logits, values):
        self.calls.append(("advance", np.asarray(logits).shape, np.asarray(values).shape))
        return self._leaves()

    def gumbel_result(self):
        self.calls.append(("result",))
        return (np.zeros((self.k, 65), np.int32), np.zeros((self.k, 65), F), np.zeros(self.k, np.int32),
                np.zeros((self.k, 65), F))

    def guided_end(self):
        self.calls.append(("end",))


def test_wrapper_checks_come_before_the_native_call():
    from envpool_amd.pgx import OthelloGymnasiumEnvPool

    env = object.__new__(OthelloGymnasiumEnvPool)
    env._pool = _Recorder()
    ids = np.array([2, 0, 1], np.int32)
    for kw in BAD:
        with pytest.raises(ValueError, match="gumbel_begin"):
            env.gumbel_search(ids, **kw)
        with pytest.raises(ValueError, match="gumbel_begin"):
            env.guided_search(ids, policy="gumbel", **kw)
    for noise in (np.zeros((2, 65), F), np.zeros((3, 64), F), np.zeros(65, F), np.full((3, 65), np.nan, F)):
        with pytest.raises(ValueError, match="gumbel_begin: gumbel"):
            env.gumbel_search(ids, gumbel=noise)
    with pytest.raises(ValueError, match="empty"):
        env.gumbel_search(np.zeros(0, np.int32))
    with pytest.raises(ValueError, match="policy"):
        env.guided_search(ids, policy="uct")
    with pytest.raises(ValueError, match="policy='gumbel'"):
        env.guided_search(ids, max_considered=4)
    assert env._pool.calls == []
    gs = env.guided_search(ids, simulations=3, policy="gumbel", max_considered=4, seed=11, c_visit=40.0)
    assert env._pool.calls == [("begin", [2, 0, 1], 3, 4, 40.0, 0.1)]
    want = np.random.Generator(np.random.PCG64(11)).gumbel(size=(3, 65)).astype(F)
    assert env._pool.gumbel.dtype == F and np.array_equal(env._pool.gumbel, want)  # the host's seeded draw
    assert [x.shape for x in gs.leaves] == [(3, 8, 8, 2), (3, 65), (3,)]
    seen = []

    def evaluate(obs, mask, status):
        seen.append((obs.shape, mask.shape, status.shape))
        return np.zeros((3, 65), F), np.zeros(3, F)

    out = gs.run(evaluate)
    assert out._fields == ("visits", "values", "action", "weights") and len(seen) == 4  # S + 1 evaluations
    assert [c[0] for c in env._pool.calls] == ["begin"] + ["advance"] * 4 + ["result", "end"]
    with pytest.raises(ValueError, match="closed"):
        gs.advance(np.zeros((3, 65), F), np.zeros(3, F))
    with pytest.raises(ValueError, match="closed"):
        gs.result()
    gs.close()  # (twice: nothing)
    assert env._pool.calls[-1] == ("end",) and len(env._pool.calls) == 7
    gs = env.gumbel_search(ids, simulations=1, gumbel=np.zeros((3, 65)))
    assert not env._pool.gumbel.any()
    gs.advance(*evaluate(*gs.leaves))
    gs.advance(*evaluate(*gs.leaves))
    with pytest.raises(ValueError, match="above simulations"):
        gs.advance(*evaluate(*gs.leaves))
    unseeded = [env.gumbel_search(ids, simulations=1) and env._pool.gumbel for _ in range(2)]
    assert not np.array_equal(unseeded[0], unseeded[1])


def test_the_other_policys_calls_are_refused_before_the_native_call():
    """A DevicePool without a native handle: whatever reaches the library fails on the missing attribute."""
    from envpool_amd.core.device_pool import DevicePool

    pool = object.__new__(DevicePool)
    zeros = (np.zeros((2, 9), F), np.zeros(2, F))
    for call in (lambda: pool.gumbel_advance(*zeros), pool.gumbel_result, lambda: pool.guided_advance(*zeros),
                 pool.guided_result):
        with pytest.raises(ValueError, match="no guided-search session"):
            call()
    pool._guided_k, pool._guided_policy = 2, "gumbel"
    for call in (lambda: pool.guided_advance(*zeros), pool.guided_result):
        with pytest.raises(ValueError, match="Gumbel search: use gumbel_"):
            call()
    pool._guided_policy = "puct"
    for call in (lambda: pool.gumbel_advance(*zeros), pool.gumbel_result,
                 lambda: pool.gumbel_advance_device(0, 0, 2, 0, 0, 0), lambda: pool.gumbel_result_device(0, 0, 0, 0)):
        with pytest.raises(ValueError, match="PUCT guided search: use guided_"):
            call()


def test_exported_symbols_and_header_agree():
    from envpool_amd.core import native

    header = open(os.path.join(ROOT, "include", "envpool_amd.h")).read()
    for stem in ("begin", "advance", "result"):
        for name in (f"epa_gumbel_{stem}", f"epa_gumbel_{stem}_device"):
            assert name in native.EXPORTED_SYMBOLS and f"int {name}(" in header
