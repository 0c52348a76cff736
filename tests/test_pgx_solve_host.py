"""PGX exact solver, CPU side: the solver of envpool_amd/csrc/pgx_solve.hip.h built for the host by g++ (a harness that
walks a wave's lanes as loops: the top tree, the lockstep rounds, the combine) against a brute force that shares nothing
with it -- a plain recursive minimax over pgx::Step without pruning (tests/cpu_harness/pgx_solve_brute.cpp) --, in
value, q, action and status; and the argument checks of the Python wrappers, which come before any native call.

The positions: 70 envs per set (pool seeds 11 + e), env 33 marked over; TicTacToe to the end of the game from 2 and 4
random plies in; ConnectFour, Hex and Othello at horizons from 3 random plies in; Othello to the end of the game from
LATE_PLIES plies in; and two hand-made positions per game, because the horizon values of random early positions are
all zeros."""
import ctypes

import numpy as np
import pytest

from pgx_solve_util import (DEPTHS, GAMES, LATE_PLIES, SOLVE_MAX_DEPTH, brute_solve, build, hand_made, host_playout,
                            host_reset, host_rolled, host_solve)
from pgx_util import ACTIONS

N, POOL_SEED, SEED, OVER = 70, 11, 15, 33
HEX_DEEP_ROWS = 24  # Hex at D = 3: 1.6 M positions of brute force per root


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pgx_solve")
    return {s: build(tmp, f"pgx_{s}.cpp") for s in ("host", "playout_host", "solve_host", "solve_brute")}


def both(libs, fam, hid, done, depth):
    """The harness and the brute force on the same rows, compared exactly; returns the harness's five arrays."""
    got, broken = host_solve(libs["solve_host"], fam, hid, done, depth)
    want, full = brute_solve(libs["solve_brute"], fam, hid, done, depth)
    for name, g, w in zip(("value", "q", "action", "status"), got, want):
        assert np.array_equal(g, w), (fam, depth, name, np.flatnonzero((g != w).reshape(len(hid), -1).any(1)))
    assert not broken.any()
    value, q, action, status, nodes = got
    run = status == 0
    assert np.array_equal(run, np.asarray(done) == 0) and (status[~run] == 2).all()
    assert (value[~run] == 0).all() and (action[~run] == -1).all() and (q[~run] == -128).all()
    assert (nodes[~run] == 0).all()
    assert (q[run].max(1) == value[run]).all() and set(np.unique(value[run])) <= {-1, 0, 1}
    assert (q[run, action[run]] == value[run]).all()
    assert ((nodes[run] > 1) & (nodes[run] <= full[run])).all()  # alpha-beta visits no more than the full tree
    return got


def early(libs, fam):
    """The game's positions a few plies in, env OVER marked over: [(hidden, done)]."""
    if fam == "TicTacToe":
        h0, d0 = host_reset(libs["host"], fam, N, POOL_SEED)
        sets = [host_playout(libs["playout_host"], fam, h0, d0, plies, SEED) for plies in (2, 4)]
    else:
        sets = [host_rolled(libs["host"], fam, N, POOL_SEED, 3)]
    for _, done in sets:
        assert not done.any()
        done[OVER] = 1
    return sets


@pytest.mark.parametrize("fam", GAMES)
def test_harness_equals_the_brute_force(libs, fam):
    values, running = [], 0
    for hid, done in early(libs, fam):
        for depth in DEPTHS[fam]:
            rows = slice(0, HEX_DEEP_ROWS) if (fam, depth) == ("Hex", 3) else slice(None)
            got = both(libs, fam, hid[rows], done[rows], depth)
            values += list(got[0][got[3] == 0])
            assert (got[3] == 2).sum() == (0 if rows.stop else 1)  # the root that is over
        running += int((done == 0).sum())
    for words, depth, value, shallower in hand_made(fam):
        got = both(libs, fam, words[None], [0], depth)
        assert got[0][0] == value and (got[1][0] != -128).sum() > 1, (fam, depth, got)
        assert both(libs, fam, words[None], [0], depth - 1)[0][0] == shallower  # not within fewer plies
        values.append(got[0][0])
        running += 1
    assert running >= 20
    assert 1 in values and -1 in values


def late_othello(libs):
    h0, d0 = host_reset(libs["host"], "Othello", N, POOL_SEED)
    hid, done = host_playout(libs["playout_host"], "Othello", h0, d0, LATE_PLIES, SEED)
    done[OVER] = 1
    return hid, done


def test_late_othello_to_the_end_of_the_game(libs):
    hid, done = late_othello(libs)
    assert (done == 0).sum() >= 20
    got = both(libs, "Othello", hid, done, 0)
    values = got[0][got[3] == 0]
    assert (values == 1).any() and (values == -1).any()
    full = brute_solve(libs["solve_brute"], "Othello", hid, done, 0)[1]
    assert 10**6 < full.sum() < 10**7  # what LATE_PLIES was chosen for


def test_max_nodes_gives_up_and_the_bytes_repeat(libs):
    hid, done = late_othello(libs)
    lib = libs["solve_host"]
    first, _ = host_solve(lib, "Othello", hid, done, 0)
    again, _ = host_solve(lib, "Othello", hid, done, 0)
    for g, w in zip(first, again):
        assert g.tobytes() == w.tobytes()
    # a row does not depend on the other rows of the call
    perm = np.random.default_rng(4).permutation(N)
    for g, w in zip(host_solve(lib, "Othello", hid[perm], done[perm], 0)[0], first):
        assert np.array_equal(g, w[perm])
    # max_nodes = 1: every running root has at least two plies left (a full tree above 2 positions) and is given up
    value, q, action, status, nodes = host_solve(lib, "Othello", hid, done, 0, max_nodes=1)[0]
    run = done == 0
    assert (status[run] == 1).all() and (status[~run] == 2).all()
    assert (value == 0).all() and (action == -1).all() and (q == -128).all() and (nodes[run] > 1).all()
    # a budget between the smallest and the largest tree: some rows of each kind, solved rows as without a budget
    budget = int(np.median(first[4][run]))
    tight = host_solve(lib, "Othello", hid, done, 0, max_nodes=budget)[0]
    gave = tight[3] == 1
    assert gave.any() and (tight[3] == 0).any()
    assert np.array_equal(gave, run & (first[4] > budget))
    for g, w in zip(tight[:3], first[:3]):
        assert np.array_equal(g[~gave], w[~gave])
    assert host_solve(lib, "Othello", hid, done, 0, max_nodes=budget)[0][4].tobytes() == tight[4].tobytes()


def test_hex_swap_and_the_cap(libs):
    """Hex one stone in: the swap (action 121) is a root action like any other.  The cap: 128 plies hold a whole game
    of Hex (121 cells and the swap) and Othello (60 placements, never two passes in a row before the last ply), and a
    root's stacks are 64 lanes x 80 bytes per ply."""
    hid, done = host_rolled(libs["host"], "Hex", 4, POOL_SEED, 1)
    got = both(libs, "Hex", hid, done, 2)
    assert (got[1][:, 121] == 0).all() and ((got[1] != -128).sum(1) == 121).all()
    lib = libs["solve_host"]
    assert lib.pgx_solve_max_depth() == SOLVE_MAX_DEPTH >= max(122, 60 + 61)
    lib.pgx_solve_stack_bytes.restype = ctypes.c_longlong
    assert lib.pgx_solve_stack_bytes(0) == 128 * 64 * 80 and lib.pgx_solve_stack_bytes(6) == 6 * 64 * 80


# ---- argument checks ----------------------------------------------------------------------------------------------
BAD = [dict(depth=-1), dict(depth=129), dict(depth=1.5), dict(max_nodes=0), dict(max_nodes=-3), dict(max_nodes=2**63)]


def test_check_solve():
    from envpool_amd.core import native

    ids = native.check_solve([[3, 1], [2, 2]], 0, 1 << 20)
    assert ids.dtype == np.int32 and ids.tolist() == [3, 1, 2, 2]  # ids may repeat
    for depth, max_nodes in ((0, 1), (128, 2**63 - 1), (1, 1 << 20)):
        native.check_solve([0], depth, max_nodes)
    assert native.SOLVE_MAX_DEPTH == SOLVE_MAX_DEPTH and native.SOLVE_ILLEGAL == -128
    for kw in BAD:
        with pytest.raises(ValueError, match="solve"):
            native.check_solve([0], **{**dict(depth=0, max_nodes=1 << 20), **kw})
    with pytest.raises(ValueError, match="empty"):
        native.check_solve(np.zeros(0, np.int32), 0, 1 << 20)
    assert {"epa_solve", "epa_solve_device"} <= set(native.EXPORTED_SYMBOLS)


class _Recorder:
    def __init__(self):
        self.calls = []

    def solve(self, env_ids, depth, max_nodes):
        self.calls.append((np.asarray(env_ids), depth, max_nodes))
        k = len(env_ids)
        return (np.zeros(k, np.int8), np.zeros((k, 65), np.int8), np.zeros(k, np.int32), np.zeros(k, np.uint8),
                np.zeros(k, np.int64))


def test_wrapper_checks_come_before_the_native_call():
    from envpool_amd.pgx import OthelloGymnasiumEnvPool

    env = object.__new__(OthelloGymnasiumEnvPool)
    env._pool = _Recorder()
    ids = np.array([2, 0, 1], np.int32)
    out = env.solve(ids, depth=6, max_nodes=1000)
    assert out._fields == ("value", "q", "action", "status", "nodes")
    assert out.value.shape == (3,) and out.q.shape == (3, 65) and out.nodes.dtype == np.int64
    assert len(env._pool.calls) == 1
    assert np.array_equal(env._pool.calls[0][0], ids) and env._pool.calls[0][1:] == (6, 1000)
    for kw in BAD:
        with pytest.raises(ValueError, match="solve"):
            env.solve(ids, **kw)
    with pytest.raises(ValueError, match="empty"):
        env.solve(np.zeros(0, np.int32))
    assert len(env._pool.calls) == 1


def test_a_family_without_solve_raises():
    """HasSolve is false for every family but PGX: the Python side of it, without a device -- a pool whose engine
    states no actions, and a pool with its own executor (no `solve` at all)."""
    from envpool_amd.classic_control import CartPoleGymnasiumEnvPool
    from envpool_amd.core.device_pool import DevicePool

    class _NoActions:
        def epa_search_actions(self, handle, out):
            out._obj.value = 0
            return 0

    pool = object.__new__(DevicePool)
    pool._lib, pool._h = _NoActions(), None
    with pytest.raises(RuntimeError, match="solve not implemented for this environment"):
        pool.solve_actions()
    env = object.__new__(CartPoleGymnasiumEnvPool)
    env._pool = object()
    with pytest.raises(RuntimeError, match="solve not implemented for this environment"):
        env._solve(np.zeros(1, np.int32), 0, 1)
    assert ACTIONS["Othello"] == 65
