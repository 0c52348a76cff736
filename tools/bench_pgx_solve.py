"""PGX exact solver, positions visited per second on one MI355X, beside the same rows through the g++ harness of the
same header (tests/cpu_harness/pgx_solve_host.cpp) on one host core:

  Othello      k late positions (`--othello-plies` random plies in, by committed playouts), D = 0: to the end of the game
  ConnectFour  k positions `--connect-plies` random plies in, D = 8

A rate is `nodes` summed over the rows -- the positions the solver visited, which the kernel and the harness count
alike -- over the time of the call: for the GPU a host clock around `pool.solve` (launch, kernel, the copy of the five
result arrays and the stream synchronisation), the median of `--repeats` calls after one warm-up call; for the harness a
host clock around the first `--host-rows` rows (the harness is single-threaded and would need minutes for all rows; the
rate is per position).  `lane_turns_used` is counted by the harness on those rows: the positions visited over the turns
the waves' lanes had (64 lanes x 512 turns x the lockstep rounds run) -- how evenly alpha-beta's uneven subtrees fill a
wave, whatever the machine.  At D = 0 a root's stacks are 640 KiB and 3276 roots fit the 2 GiB of scratch, so k = 4096 is
solved in two calls, both inside the timed window.  Rows that were given up or are over are counted and reported.

    python tools/bench_pgx_solve.py [--k 4096] [--repeats 3] [--host-rows 64] [--othello-plies 48] [--connect-plies 6]
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


def harness():
    out = os.path.join(tempfile.mkdtemp(prefix="pgx_solve_"), "libpgxsolvehost.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "cpu_harness", "pgx_solve_host.cpp"), "-o", out], check=True)
    return ctypes.CDLL(out)


def host_solve(lib, fam, st, n_act, depth, max_nodes):
    hid = np.ascontiguousarray(st[:, 2:], np.int32)
    done = np.ascontiguousarray(st[:, 1] != 0, np.uint8)
    k = len(hid)
    value, q = np.zeros(k, np.int8), np.zeros((k, n_act), np.int8)
    action, status = np.zeros(k, np.int32), np.zeros(k, np.uint8)
    nodes, broken, rounds = np.zeros(k, np.int64), np.zeros(k, np.uint8), np.zeros(k, np.int64)
    ptr = [a.ctypes.data_as(ctypes.c_void_p) for a in (hid, done, value, q, action, status, nodes, broken, rounds)]
    t0 = time.perf_counter()
    rc = lib.pgx_solve(CODE[fam], k, ptr[0], ptr[1], depth, ctypes.c_longlong(max_nodes), *ptr[2:])
    dt = time.perf_counter() - t0
    assert rc == 0, rc
    # the share of the lanes' turns that visited a position: a round gives each of a wave's 64 lanes up to
    # pgx_solve_slice() turns, and lasts until its busiest lane has used its own
    busy = nodes.sum() / max(64 * lib.pgx_solve_slice() * rounds.sum(), 1)
    return (value, q, action, status, nodes), dt, float(busy)


def gpu_solve(pool, ids, depth, max_nodes):
    """pool.solve in as few calls as the scratch limit allows."""
    per_call = SCRATCH // ((depth or 128) * STACK_BYTES_PER_PLY)
    parts = [pool.solve(ids[i:i + per_call], depth, max_nodes) for i in range(0, len(ids), per_call)]
    return tuple(np.concatenate(x) for x in zip(*parts)), len(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-rows", type=int, default=64)
    ap.add_argument("--othello-plies", type=int, default=48)
    ap.add_argument("--connect-plies", type=int, default=6)
    ap.add_argument("--max-nodes", type=int, default=1 << 40)
    args = ap.parse_args()
    from envpool_amd.core.device_pool import DevicePool

    lib = harness()
    for fam, plies, depth in (("Othello", args.othello_plies, 0), ("ConnectFour", args.connect_plies, 8)):
        pool = DevicePool(fam, args.k, seed=0)
        ids = np.arange(args.k, dtype=np.int32)
        pool.reset(ids)
        pool.recv_dict()
        pool.playout(ids, 1, plies, 15, commit=True)
        st = pool.get_state()
        n_act = pool.solve_actions()
        got, calls = gpu_solve(pool, ids, depth, args.max_nodes)  # the warm-up call
        times = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            again, _ = gpu_solve(pool, ids, depth, args.max_nodes)
            times.append(time.perf_counter() - t0)
            assert all(np.array_equal(a, b) for a, b in zip(again, got))
        rows = min(args.host_rows, args.k)
        want, host_s, busy = host_solve(lib, fam, st[:rows], n_act, depth, args.max_nodes)
        equal = all(np.array_equal(g[:rows], w) for g, w in zip(got, want))
        gpu_s = float(np.median(times))
        gpu_rate, host_rate = got[4].sum() / gpu_s, want[4].sum() / max(host_s, 1e-9)
        print(json.dumps({"game": fam, "k": args.k, "plies_in": plies, "depth": depth, "calls": calls,
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
