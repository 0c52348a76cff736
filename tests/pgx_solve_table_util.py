"""Shared helpers of the tests of the PGX solver's transposition tables (solve table_bits=): the g++ harness of
pgx_solve.hip.h with tables (tests/cpu_harness/pgx_solve_table_host.cpp) and the positions both test files use.  The
positions, the brute force and the table-less harness come from pgx_solve_util.py."""
import ctypes

import numpy as np

from pgx_solve_util import BIG, LATE_PLIES, _ptr, build, host_playout, host_reset, host_rolled
from pgx_util import ACTIONS, CODE

NAMES = ("value", "q", "action", "status", "nodes")
MAX_TABLE_BITS = 16
N, POOL_SEED, SEED, OVER = 70, 11, 15, 33  # the sets of test_pgx_solve_host.py
HEX_DEEP_ROWS = 24  # Hex at D = 3: 1.6 M positions of brute force per root
# ConnectFour DEEP_PLIES random plies in (`rolled` over DEEP_POOL envs, pool seeds 11 + e), to the end of the game
# (D = 0).  The full trees are too large for the brute force; the table-less harness, which test_pgx_solve_host.py pins
# to the brute force, is the reference.  Many of these roots need 10^7 positions and more without a table, so the rows
# are chosen, on the CPU with the two harnesses, among the first 700 envs:
#   DEEP_ENVS  8 rows of 361,493 .. 1,100,981 positions without a table (at most 188 rounds, so a wave is done with one
#              in well under a second)
#   GIVE_ENVS  "given up becomes solved": at max_nodes = GIVE_NODES the table-less solve gives these rows up, the solve
#              with table_bits = GIVE_BITS solves them.  max_nodes is looked at between rounds of 512 positions per
#              lane, so the rows are away from it on both sides: `nodes` at BIG is above 4 GIVE_NODES without a table
#              and below GIVE_NODES / 2 with it --
#                env               222        299        559        646
#                table-less  2,601,378  2,878,365  5,834,931  2,525,699
#                table_bits 12 162,528    300,386    303,673    223,497
DEEP_PLIES, DEEP_POOL = 24, 700
DEEP_ENVS = [15, 32, 49, 147, 152, 473, 620, 639]
GIVE_ENVS = [222, 299, 559, 646]
GIVE_NODES, GIVE_BITS = 620_000, 12
# Total positions (`nodes` summed over the running rows) by the harnesses, table-less -> table_bits = 10:
#   TicTacToe, the empty board (1 row), D = 0        47,518 -> 25,018
#   ConnectFour, the DEEP_ENVS rows, D = 0           5,322,875 -> 1,601,128
#   Othello, LATE_PLIES plies in (69 rows), D = 0    658,418 -> 600,095
# (A table is private to one lane of the root's wave and sees that lane's share of the frontier only, so the gain is
# smaller than that of one table per root; it grows with the depth of the lanes' subtrees.)


def build_libs(tmp):
    return {s: build(tmp, f"pgx_{s}.cpp")
            for s in ("host", "playout_host", "solve_host", "solve_brute", "solve_table_host")}


def table_solve(lib, fam, hid, done, depth, table_bits, max_nodes=BIG):
    """The harness with tables: (value, q, action, status, nodes), broken."""
    hid, done = np.ascontiguousarray(hid, np.int32), np.ascontiguousarray(done, np.uint8)
    k, a = len(hid), ACTIONS[fam]
    value, q = np.full(k, 99, np.int8), np.full((k, a), 99, np.int8)
    action, status = np.full(k, -7, np.int32), np.full(k, 99, np.uint8)
    nodes, broken = np.full(k, -7, np.int64), np.zeros(k, np.uint8)
    rc = lib.pgx_solve_table(CODE[fam], k, _ptr(hid), _ptr(done), int(depth), ctypes.c_longlong(int(max_nodes)),
                             int(table_bits), _ptr(value), _ptr(q), _ptr(action), _ptr(status), _ptr(nodes),
                             _ptr(broken), None)
    assert rc == 0, rc
    return (value, q, action, status, nodes), broken


def key_test(lib, fam, stored, probed, plies, lo, hi):
    """Stores `stored` (hidden words) with plies[0] plies left and the bounds in a table of one entry, then looks
    `probed` up with plies[1] plies left: None on a miss, the bounds found on a hit."""
    stored, probed = np.ascontiguousarray(stored, np.int32), np.ascontiguousarray(probed, np.int32)
    plies, got = (ctypes.c_int * 2)(*plies), (ctypes.c_int * 2)(9, 9)
    rc = lib.pgx_solve_table_key_test(CODE[fam], _ptr(stored), _ptr(probed), plies, lo, hi, got)
    assert rc in (0, 1), rc
    return (got[0], got[1]) if rc else None


def early(libs, fam):
    """The game's positions a few plies in, env OVER marked over: [(hidden, done)] (test_pgx_solve_host.py)."""
    if fam == "TicTacToe":
        h0, d0 = host_reset(libs["host"], fam, N, POOL_SEED)
        sets = [host_playout(libs["playout_host"], fam, h0, d0, plies, SEED) for plies in (2, 4)]
    else:
        sets = [host_rolled(libs["host"], fam, N, POOL_SEED, 3)]
    for _, done in sets:
        assert not done.any()
        done[OVER] = 1
    return sets


def late_othello(libs):
    h0, d0 = host_reset(libs["host"], "Othello", N, POOL_SEED)
    hid, done = host_playout(libs["playout_host"], "Othello", h0, d0, LATE_PLIES, SEED)
    done[OVER] = 1
    return hid, done


_deep = {}


def deep_connect_four(libs, envs):
    """(hidden, done) of the listed envs of the DEEP pool: all running."""
    if not _deep:
        _deep["rolled"] = host_rolled(libs["host"], "ConnectFour", DEEP_POOL, POOL_SEED, DEEP_PLIES)
    hid, done = _deep["rolled"]
    assert not done[envs].any()
    return hid[envs].copy(), done[envs].copy()


def empty_tictactoe(libs):
    return host_reset(libs["host"], "TicTacToe", 1, POOL_SEED)
