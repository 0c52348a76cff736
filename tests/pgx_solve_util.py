"""Shared helpers of the PGX solver tests: the g++ harnesses (the solver of pgx_solve.hip.h, the brute-force minimax
that shares nothing with it, the playout and replay harnesses that make positions), and the hand-made positions."""
import ctypes
import os
import subprocess

import numpy as np

from pgx_util import ACTIONS, CODE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMES = ["TicTacToe", "ConnectFour", "Hex", "Othello"]
SOLVE_MAX_DEPTH = 128
BIG = 1 << 40  # a max_nodes that no test position reaches
# the horizons of the early positions (3 plies in; TicTacToe: 2 and 4 plies in, to the end of the game)
DEPTHS = {"TicTacToe": [0], "ConnectFour": [4, 6], "Hex": [2, 3], "Othello": [4]}
# Late Othello: positions after playout(max_plies=LATE_PLIES) from the reset, solved to the end (D = 0).  Chosen on the
# CPU with the playout harness and the brute force over 70 envs (pool seeds 11 + e, playout seed 15): the full minimax
# trees have 6,949,459 positions in total at 51 plies (201,505 at 53); under the 10^7 the tests allow.
LATE_PLIES = 51


def build(tmp, source):
    out = str(tmp / ("lib" + source.replace(".cpp", ".so")))
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "cpu_harness", source), "-o", out], check=True)
    return ctypes.CDLL(out)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_solve(lib, fam, hid, done, depth, max_nodes=BIG):
    """The harness of pgx_solve.hip.h: (value, q, action, status, nodes), broken."""
    hid, done = np.ascontiguousarray(hid, np.int32), np.ascontiguousarray(done, np.uint8)
    k, a = len(hid), ACTIONS[fam]
    value, q = np.full(k, 99, np.int8), np.full((k, a), 99, np.int8)
    action, status = np.full(k, -7, np.int32), np.full(k, 99, np.uint8)
    nodes, broken = np.full(k, -7, np.int64), np.zeros(k, np.uint8)
    rc = lib.pgx_solve(CODE[fam], k, _ptr(hid), _ptr(done), int(depth), ctypes.c_longlong(int(max_nodes)), _ptr(value),
                       _ptr(q), _ptr(action), _ptr(status), _ptr(nodes), _ptr(broken), None)
    assert rc == 0, rc
    return (value, q, action, status, nodes), broken


def brute_solve(lib, fam, hid, done, depth):
    """The plain minimax: (value, q, action, status), the positions of the full trees."""
    hid, done = np.ascontiguousarray(hid, np.int32), np.ascontiguousarray(done, np.uint8)
    k, a = len(hid), ACTIONS[fam]
    value, q = np.full(k, 99, np.int8), np.full((k, a), 99, np.int8)
    action, status, nodes = np.full(k, -7, np.int32), np.full(k, 99, np.uint8), np.zeros(k, np.int64)
    rc = lib.pgx_solve_brute(CODE[fam], k, _ptr(hid), _ptr(done), int(depth), _ptr(value), _ptr(q), _ptr(action),
                             _ptr(status), _ptr(nodes))
    assert rc == 0, rc
    return (value, q, action, status), nodes


def legal_random(mask, rng):
    mask = np.asarray(mask, bool)
    return (rng.random(mask.shape) * mask + mask).argmax(1).astype(np.int32)


def rolled(step, plies):
    """`plies` seeded random legal plies of every env through `step(actions) -> legal mask` (test_gpu_pgx_search.py)."""
    rng = np.random.default_rng(2)
    mask = step(None)
    for _ in range(plies):
        mask = step(legal_random(mask, rng))
    return mask


def host_reset(host, fam, n, pool_seed):
    """The hidden words of n envs after their reset (env e's generator seeded pool_seed + e)."""
    return host_rolled(host, fam, n, pool_seed, 0)


def host_rolled(host, fam, n, pool_seed, plies):
    """The hidden words of n envs after `rolled(.., plies)` through the replay harness, and their done flags."""
    from pgx_util import KEYS, fixture

    code, words = CODE[fam], host.pgx_hidden_words(CODE[fam])
    g = fixture(f"{fam}-v1")  # (for the keys' row shapes and types)
    seeds = np.arange(pool_seed, pool_seed + n, dtype=np.int32)
    acts = []
    hid = done = None

    def step(act):
        nonlocal hid, done
        if act is not None:
            acts.append(act)
        t = len(acts)
        a = np.ascontiguousarray(np.array(acts, np.int32).reshape(t, n))
        outs = {k: np.zeros((t + 1, n) + g[k].shape[2:], g[k].dtype) for k in KEYS}
        h = np.zeros((t + 1, n, words), np.int32)
        ptrs = (ctypes.c_void_p * len(KEYS))(*[outs[k].ctypes.data for k in KEYS])
        assert host.pgx_replay(code, n, t, _ptr(seeds), _ptr(a), 2**31 - 1, ptrs, _ptr(h)) == 0
        hid, done = h[-1].copy(), outs["done"][-1].reshape(n).astype(np.uint8)
        return outs["info:legal_action_mask"][-1].reshape(n, -1)

    rolled(step, plies)
    return hid, done


def host_playout(play, fam, hid, done, max_plies, seed):
    """The positions after one playout of at most max_plies plies from each of the rows (env ids 0 .. n-1)."""
    hid, done = np.ascontiguousarray(hid, np.int32), np.ascontiguousarray(done, np.uint8)
    n, w = hid.shape
    ret, plies, status = np.zeros((n, 2), np.float32), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    hid_out, done_out = np.zeros((n, w), np.int32), np.zeros(n, np.uint8)
    ids = np.arange(n, dtype=np.int32)
    assert play.pgx_playout(CODE[fam], n, _ptr(hid), _ptr(done), _ptr(ids), 1, max_plies, ctypes.c_uint64(seed),
                            _ptr(ret), _ptr(plies), _ptr(status), _ptr(hid_out), _ptr(done_out)) == 0
    return hid_out, done_out


def _board(cells, mine, theirs, a, b):
    w = np.zeros(cells, np.int32) if (a, b) == (1, -1) else np.full(cells, -1, np.int32)
    w[list(mine)] = a
    w[list(theirs)] = b
    return w


def hand_made(fam):
    """[(hidden words, D, the value at D, the value at D - 1)]: per game a forced win in 3 plies and a forced loss in 2
    for the side to move, each with more than one legal move.
      TicTacToe    X (color 0) on 0 4, O on 1 8: X plays 6 and threatens 2 and 3; then the same with O to move.
      ConnectFour  bottom row O X X . . . O with X to move: column 4 makes an open three; then O to move against it.
      Hex          color 0 (joins x = 0 to x = 10) holds (0..8, 5): (9, 5) reaches both (10, 4) and (10, 5); then
                   color 1 to move against the chain (0..9, 5).
      Othello      the mover takes (0, 1) from (0, 0); the other's one stone (7, 1) has one move, (7, 3), and the mover
                   wipes row 7 out from (7, 0).  Then a mover whose one stone (3, 3) has two moves, and after either
                   the other side takes the whole line."""
    if fam == "TicTacToe":
        win = np.r_[_board(9, [0, 4], [1, 8], 0, 1), 0, 0]
        loss = np.r_[_board(9, [0, 4, 6], [1, 8], 0, 1), 1, 1]
    elif fam == "ConnectFour":
        win = np.r_[_board(42, [37, 38], [35, 41], 0, 1), 0, 1]
        loss = np.r_[_board(42, [37, 38, 39], [35, 41], 0, 1), 1, 0]
    elif fam == "Hex":
        chain = [x * 11 + 5 for x in range(9)]
        edge = [x * 11 for x in range(9)]
        win = np.r_[_board(121, chain, edge, 1, -1), 18, 0]
        loss = np.r_[_board(121, edge, chain + [9 * 11 + 5], 1, -1), 19, 1]
    else:
        win = np.r_[_board(64, [2, 58, 60], [1, 57], 1, -1), 0, 0, 0]
        loss = np.r_[_board(64, [27], [28, 30, 35, 51], 1, -1), 1, 1, 0]
    return [(win.astype(np.int32), 3, 1, 0), (loss.astype(np.int32), 2, -1, 0)]
