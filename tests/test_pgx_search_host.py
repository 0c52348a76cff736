"""PGX tree search, CPU side: the search of envpool_amd/csrc/pgx_search.hip.h built for the host by g++ (a harness that
walks a wave's lanes as loops) against the contract restated in numpy (pgx_search_util.py), which keeps the tree in
Python, takes every expansion step from the reference-pinned `pgx_replay` of the PGX host harness and every leaf
value from the `pgx_playout` harness (repeats t * R .. t * R + R - 1), and shares no code with the header; and the
argument checks of the Python wrappers, which come before any native call."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from pgx_search_util import Pos, puct_search
from pgx_util import ACTIONS, CODE, KEYS, fixture, game

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMES = ["TicTacToe-v1", "ConnectFour-v1", "Hex-v1", "Othello-v1"]
SEED = 15
ENV_ID = 70003  # the global id the leaf playouts are keyed by
S, R = 24, 4


# ---- the three harnesses ----------------------------------------------------------------------------------------
def _build(tmp, source, name):
    out = str(tmp / name)
    # no fast-math, no contraction: the score is float32, operation by operation
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "cpu_harness", source), "-o", out], check=True)
    return ctypes.CDLL(out)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pgx_search")
    return (_build(tmp, "pgx_host.cpp", "libpgxhost.so"), _build(tmp, "pgx_playout_host.cpp", "libpgxplayouthost.so"),
            _build(tmp, "pgx_search_host.cpp", "libpgxsearchhost.so"))


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Replayed:
    """Positions of one env column of a fixture, named by their action sequence from the reset: expansion by
    pgx_replay, leaf values by pgx_playout.  Counts what it saw for the tests' own assertions."""

    def __init__(self, libs, tid, column, leaf_playouts=R, max_plies=0, seed=SEED):
        self.host, self.play, _ = libs
        self.tid, self.code = tid, CODE[game(tid)]
        self.g = fixture(tid)
        self.column = column
        self.r, self.max_plies, self.seed = leaf_playouts, max_plies, seed
        self.words = self.host.pgx_hidden_words(self.code)
        self.playouts = 0
        self.cut = 0
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
        pos = Pos(mask=outs["info:legal_action_mask"][-1, 0].astype(bool), done=bool(outs["done"][-1, 0]),
                  mover=int(outs["info:current_player"][-1, 0]), key=(tuple(seq), hid[-1, 0].copy()))
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

    def leaf(self, pos, t):
        n = (t + 1) * self.r
        ret, plies, status = np.zeros((n, 2), np.float32), np.zeros(n, np.int32), np.zeros(n, np.uint8)
        hid_out, done_out = np.zeros((n, self.words), np.int32), np.zeros(n, np.uint8)
        hid, done = np.ascontiguousarray(pos.key[1], np.int32), np.zeros(1, np.uint8)
        ids = np.array([ENV_ID], np.int32)
        assert self.play.pgx_playout(self.code, 1, _ptr(hid), _ptr(done), _ptr(ids), n, self.max_plies,
                                     ctypes.c_uint64(self.seed), _ptr(ret), _ptr(plies), _ptr(status), _ptr(hid_out),
                                     _ptr(done_out)) == 0
        ret, status = ret[-self.r:], status[-self.r:]
        assert np.array_equal(ret[:, 0], -ret[:, 1]) and set(np.unique(ret)) <= {-1.0, 0.0, 1.0}  # zero-sum
        self.playouts += self.r
        self.cut += int((status == 1).sum())
        return int(ret[:, 0].sum())


def host_search(libs, tid, pos, simulations, leaf_playouts, c_puct, max_plies=0, seed=SEED):
    lib = libs[2]
    n_act = ACTIONS[game(tid)]
    hid, done = np.ascontiguousarray(pos.key[1], np.int32), np.array([pos.done], np.uint8)
    ids = np.array([ENV_ID], np.int32)
    visits, returns = np.full((1, n_act), -7, np.int32), np.full((1, n_act), -7, np.int32)
    action, nodes = np.full(1, -7, np.int32), np.zeros(1, np.int32)
    rc = lib.pgx_search(CODE[game(tid)], 1, _ptr(hid), _ptr(done), _ptr(ids), simulations, leaf_playouts,
                        ctypes.c_float(c_puct), max_plies, ctypes.c_uint64(seed), _ptr(visits), _ptr(returns),
                        _ptr(action), _ptr(nodes))
    assert rc == 0
    return visits[0], returns[0], int(action[0]), int(nodes[0])


def both(libs, game_, pos, simulations, leaf_playouts, c_puct, max_plies=0):
    """The numpy restatement and the harness from `pos`, compared exactly; returns the harness's result."""
    want = puct_search(pos, game_.expand, game_.leaf, simulations, leaf_playouts, c_puct)
    got = host_search(libs, game_.tid, pos, simulations, leaf_playouts, c_puct, max_plies)
    assert np.array_equal(got[0], want[0]), (game_.tid, "visits", got[0], want[0])
    assert np.array_equal(got[1], want[1]), (game_.tid, "returns", got[1], want[1])
    assert got[2] == want[2] and got[3] == want[3], (game_.tid, got[2:], want[2:])
    assert got[0].sum() == (0 if pos.done else simulations)
    assert (got[0][~pos.mask] == 0).all() and (got[1][~pos.mask] == 0).all()
    return got


def mid_row(g, column):
    """A fixture row a few plies into a game at which the column's env is not over."""
    return next(t for t in range(4, len(g["done"])) if not g["done"][t, column] and g["elapsed_step"][t, column] >= 3)


@pytest.mark.parametrize("c_puct", [1.25, 0.0])
@pytest.mark.parametrize("mid", [False, True])
@pytest.mark.parametrize("tid", GAMES)
def test_host_search_equals_the_numpy_restatement(libs, tid, mid, c_puct):
    game_ = Replayed(libs, tid, column=2 if mid else 1)
    pos = game_.fixture_row(mid_row(game_.g, 2) if mid else 0)
    assert not pos.done
    got = both(libs, game_, pos, S, R, c_puct)
    assert got[2] >= 0 and pos.mask[got[2]]
    assert game_.playouts > 0
    if c_puct > 0 and pos.mask.sum() > 4:
        assert (got[0] > 0).sum() > 1  # exploration spreads the visits


def test_a_root_that_is_over_reports_zeros(libs):
    game_ = Replayed(libs, "TicTacToe-v1", column=0)
    t0 = int(np.flatnonzero(game_.g["done"][:, 0])[0])
    pos = game_.fixture_row(t0)
    assert pos.done
    got = both(libs, game_, pos, S, R, 1.25)
    assert got[2] == -1 and not got[0].any() and not got[1].any()


def test_exhausted_tree_revisits_terminal_nodes(libs):
    """TicTacToe with three empty cells: at most 1 + 3 + 6 + 6 nodes, so most of 64 simulations end in a node whose
    game is over and back up R * term0 again."""
    game_ = Replayed(libs, "TicTacToe-v1", column=0)
    pos, _ = game_.at([0, 1, 2, 4, 3, 5])
    assert not pos.done and pos.mask.sum() == 3
    got = both(libs, game_, pos, 64, R, 1.25)
    assert got[3] <= 16 and len(game_.expanded) == got[3] - 1
    assert game_.playouts < 16 * R


def test_hex_swap_and_second_slots(libs):
    """Hex one stone in: 120 cells and the swap (action 121) are legal, all of them in play with a large c_puct and
    S > 121: the second action of a lane is scored, picked, expanded and backed up."""
    game_ = Replayed(libs, "Hex-v1", column=0, leaf_playouts=1)
    pos, _ = game_.at([60])
    assert pos.mask[121] and pos.mask.sum() == 121
    got = both(libs, game_, pos, 128, 1, 100.0)
    assert got[0][121] >= 1 and 121 in game_.expanded and (got[0][pos.mask] >= 1).all()


def find_forced_pass(libs):
    """The first Othello position of seeded random legal play at which the pass is the only legal move."""
    game_ = Replayed(libs, "Othello-v1", column=0)
    rng = np.random.default_rng(5)
    for _ in range(400):
        seq = []
        pos, _ = game_.at(seq)
        while not pos.done:
            if pos.mask[64]:
                assert pos.mask.sum() == 1
                return game_, pos
            seq.append(int(rng.choice(np.flatnonzero(pos.mask))))
            pos, _ = game_.at(seq)
    raise AssertionError("no forced pass found")


def test_othello_forced_pass(libs):
    """The pass (action 64) is lane 0's second slot; here it is the only legal move of the root."""
    game_, pos = find_forced_pass(libs)
    got = both(libs, game_, pos, S, R, 1.25)
    assert got[0][64] == S and got[2] == 64 and got[3] > 2


@pytest.mark.parametrize("tid", ["ConnectFour-v1", "Othello-v1"])
def test_max_plies_cuts_the_leaf_playouts(libs, tid):
    game_ = Replayed(libs, tid, column=3, max_plies=5)
    pos = game_.fixture_row(0)
    both(libs, game_, pos, S, R, 1.25, max_plies=5)
    assert game_.cut > 0
    uncut = Replayed(libs, tid, column=3)
    assert not np.array_equal(host_search(libs, tid, pos, S, R, 1.25, 5)[1], host_search(libs, tid, pos, S, R, 1.25)[1])
    both(libs, uncut, pos, S, R, 1.25)
    assert uncut.cut == 0


def test_node_layout(libs):
    """80 bytes of State and term0, then three int32 arrays of A rounded up to whole 16-byte words."""
    for name, n_act in ACTIONS.items():
        assert libs[2].pgx_search_node_bytes(CODE[name]) == 80 + 3 * 4 * ((n_act + 3) // 4 * 4)


# ---- argument checks ----------------------------------------------------------------------------------------------
BAD = [dict(simulations=0), dict(simulations=4097), dict(leaf_playouts=0), dict(leaf_playouts=65),
       dict(simulations=1025, leaf_playouts=4), dict(simulations=65, leaf_playouts=64), dict(max_plies=-1),
       dict(max_plies=257), dict(c_puct=-0.5), dict(c_puct=float("nan")), dict(c_puct=float("inf")),
       dict(c_puct=1e39)]


def test_check_search():
    from envpool_amd.core import native

    ids = native.check_search([[3, 1], [2, 2]], 64, 8, 1.25, 0)
    assert ids.dtype == np.int32 and ids.tolist() == [3, 1, 2, 2]  # ids may repeat
    for s, r in ((4096, 1), (64, 64), (1, 1), (1024, 4)):
        native.check_search([0], s, r, 0.0, 256)
    base = dict(simulations=64, leaf_playouts=8, c_puct=1.25, max_plies=0)
    for kw in BAD:
        with pytest.raises(ValueError, match="search"):
            native.check_search([0], **{**base, **kw})
    with pytest.raises(ValueError, match="empty"):
        native.check_search(np.zeros(0, np.int32), **base)


class _Recorder:
    def __init__(self):
        self.calls = []

    def search(self, env_ids, simulations, leaf_playouts, c_puct, max_plies, seed):
        self.calls.append((np.asarray(env_ids), simulations, leaf_playouts, c_puct, max_plies, seed))
        k = len(env_ids)
        return np.zeros((k, 65), np.int32), np.zeros((k, 65), np.int32), np.zeros(k, np.int32)


def test_wrapper_checks_come_before_the_native_call():
    from envpool_amd.pgx import OthelloGymnasiumEnvPool

    env = object.__new__(OthelloGymnasiumEnvPool)
    env._pool = _Recorder()
    ids = np.array([2, 0, 1], np.int32)
    out = env.search(ids, simulations=16, leaf_playouts=2, c_puct=0.5, max_plies=9, seed=5)
    assert out._fields == ("visits", "returns", "action")
    assert out.visits.shape == (3, 65) and out.returns.shape == (3, 65) and out.action.shape == (3,)
    assert len(env._pool.calls) == 1
    assert np.array_equal(env._pool.calls[0][0], ids) and env._pool.calls[0][1:] == (16, 2, 0.5, 9, 5)
    for kw in BAD:
        with pytest.raises(ValueError, match="search"):
            env.search(ids, **kw)
    with pytest.raises(ValueError, match="empty"):
        env.search(np.zeros(0, np.int32))
    assert len(env._pool.calls) == 1
