"""PGX exact solver, positions visited per second on one MI355X, beside the same rows through the g++ harness of the
same header (tests/cpu_harness/pgx_solve_host.cpp) on one host core:

  Othello      k late positions (`--othello-plies` random plies in, by committed playouts), D = 0: to the end of the game
  ConnectFour  k positions `--connect-plies` random plies in, D = 8
  ConnectFour  `--deep-k` positions `--deep-plies` random plies in, D = 0: to the end of the game, every root with at
               most `--deep-max-nodes` positions (the trees of some of these roots have 10^8 positions and more)

`--table-bits b` (1 .. 16) solves with the lanes' transposition tables (solve table_bits=) and compares with the harness
that has them (tests/cpu_harness/pgx_solve_table_host.cpp); without it, or with 0, the calls and the harness are the
table-less ones.

A rate is `nodes` summed over the rows -- the positions the solver visited, which the kernel and the harness count
alike -- over the time of the call: for the GPU a host clock around `pool.solve` (launch, kernel, the copy of the five
result arrays and the stream synchronisation), the median of `--repeats` calls after one warm-up call; for the harness a
host clock around the first `--host-rows` rows (the harness is single-threaded and would need minutes for all rows; the
rate is per position).  `lane_turns_used` is counted by the harness on those rows: the positions visited over the turns
the waves' lanes had (64 lanes x 512 turns x the lockstep rounds run) -- how evenly alpha-beta's uneven subtrees fill a
wave, whatever the machine.  At D = 0 a root's stacks are 640 KiB and 3276 roots fit the 2 GiB of scratch, so k = 4096 is
solved in two calls, both inside the timed window; a root's tables are 64 x 2^b x 32 bytes more.  Rows that were given
up or are over are counted and reported.

    python tools/bench_pgx_solve.py [--k 4096] [--repeats 3] [--host-rows 64] [--othello-plies 48] [--connect-plies 6]
                                    [--deep-k 64] [--deep-plies 24] [--deep-max-nodes 4194304] [--table-bits 0]
                                    [--rows othello,connect,deep]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CODE = {"TicTacToe": 0, "ConnectFour": 1, "Hex": 2, "Othello": 3}
SCRATCH = 2**31  # EPA_SEARCH_MAX_TREE_BYTES
STACK_BYTES_PER_PLY = 64 * 80


def harness(table_bits):
    out = os.path.join(tempfile.mkdtemp(prefix="pgx_solve_"), "libpgxsolvehost.so")
    source = "pgx_solve_table_host.cpp" if table_bits else "pgx_solve_host.cpp"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "cpu_harness", source), "-o", out], check=True)
    return ctypes.CDLL(out)


def host_solve(lib, fam, st, n_act, depth, max_nodes, table_bits):
    hid = np.ascontiguousarray(st[:, 2:], np.int32)
    done = np.ascontiguousarray(st[:, 1] != 0, np.uint8)
    k = len(hid)
    value, q = np.zeros(k, np.int8), np.zeros((k, n_act), np.int8)
    action, status = np.zeros(k, np.int32), np.zeros(k, np.uint8)
    nodes, broken, rounds = np.zeros(k, np.int64), np.zeros(k, np.uint8), np.zeros(k, np.int64)
    ptr = [a.ctypes.data_as(ctypes.c_void_p) for a in (hid, done, value, q, action, status, nodes, broken, rounds)]
    t0 = time.perf_counter()
    if table_bits:
        rc = lib.pgx_solve_table(CODE[fam], k, ptr[0], ptr[1], depth, ctypes.c_longlong(max_nodes), table_bits,
                                 *ptr[2:])
    else:
        rc = lib.pgx_solve(CODE[fam], k, ptr[0], ptr[1], depth, ctypes.c_longlong(max_nodes), *ptr[2:])
    dt = time.perf_counter() - t0
    assert rc == 0, rc
    # the share of the lanes' turns that visited a position: a round gives each of a wave's 64 lanes up to
    # pgx_solve_slice() turns, and lasts until its busiest lane has used its own
    busy = nodes.sum() / max(64 * lib.pgx_solve_slice() * rounds.sum(), 1)
    return (value, q, action, status, nodes), dt, float(busy)


def gpu_solve(pool, ids, depth, max_nodes, table_bits):
    """pool.solve in as few calls as the scratch limit allows."""
    per_call = SCRATCH // ((depth or 128) * STACK_BYTES_PER_PLY + (64 * 32 << table_bits if table_bits else 0))
    kw = dict(table_bits=table_bits) if table_bits else {}
    parts = [pool.solve(ids[i:i + per_call], depth, max_nodes, **kw) for i in range(0, len(ids), per_call)]
    return tuple(np.concatenate(x) for x in zip(*parts)), len(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-rows", type=int, default=64)
    ap.add_argument("--othello-plies", type=int, default=48)
    ap.add_argument("--connect-plies", type=int, default=6)
    ap.add_argument("--max-nodes", type=int, default=1 << 40)
    ap.add_argument("--deep-k", type=int, default=64)
    ap.add_argument("--deep-plies", type=int, default=24)
    ap.add_argument("--deep-max-nodes", type=int, default=1 << 22)
    ap.add_argument("--table-bits", type=int, default=0)
    ap.add_argument("--rows", default="othello,connect,deep")
    args = ap.parse_args()
    bits, rows_wanted = args.table_bits, args.rows.split(",")
    from envpool_amd.core.device_pool import DevicePool

    lib = harness(bits)
    for row, fam, plies, depth, k, max_nodes in (
            ("othello", "Othello", args.othello_plies, 0, args.k, args.max_nodes),
            ("connect", "ConnectFour", args.connect_plies, 8, args.k, args.max_nodes),
            ("deep", "ConnectFour", args.deep_plies, 0, args.deep_k, args.deep_max_nodes)):
        if row not in rows_wanted:
            continue
        pool = DevicePool(fam, k, seed=0)
        ids = np.arange(k, dtype=np.int32)
        pool.reset(ids)
        pool.recv_dict()
        pool.playout(ids, 1, plies, 15, commit=True)
        st = pool.get_state()
        n_act = pool.solve_actions()
        got, calls = gpu_solve(pool, ids, depth, max_nodes, bits)  # the warm-up call
        times = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            again, _ = gpu_solve(pool, ids, depth, max_nodes, bits)
            times.append(time.perf_counter() - t0)
            assert all(np.array_equal(a, b) for a, b in zip(again, got))
        rows = min(args.host_rows, k)
        want, host_s, busy = host_solve(lib, fam, st[:rows], n_act, depth, max_nodes, bits)
        equal = all(np.array_equal(g[:rows], w) for g, w in zip(got, want))
        gpu_s = float(np.median(times))
        gpu_rate, host_rate = got[4].sum() / gpu_s, want[4].sum() / max(host_s, 1e-9)
        print(json.dumps({"game": fam, "k": k, "plies_in": plies, "depth": depth, "table_bits": bits, "calls": calls,
                          "solved": int((got[3] == 0).sum()), "given_up": int((got[3] == 1).sum()),
                          "over": int((got[3] == 2).sum()), "nodes": int(got[4].sum()),
                          "nodes_max_row": int(got[4].max()), "gpu_s": round(gpu_s, 4),
                          "gpu_s_all": [round(t, 4) for t in times], "gpu_nodes_per_s": round(gpu_rate),
                          "host_rows": rows, "host_nodes": int(want[4].sum()), "host_s": round(host_s, 4),
                          "host_nodes_per_s_one_core": round(host_rate), "host_equals_gpu": bool(equal),
                          "lane_turns_used": round(busy, 3),
                          "gpu_over_16_host_cores": round(gpu_rate / (16 * host_rate), 3)}), flush=True)
        pool.close()


if __name__ == "__main__":
    main()
