"""Snapshot / restore / fork of a whole pool on one MI355X, timed with events on the pool's stream, beside the flat
state path (`get_state` + `set_state`) of the same envs on the same build.

    python tools/bench_snapshot.py <task-id> <num_envs> [--reps 20] [--warmup 3] [--roll 8]

One JSON line per operation: median milliseconds, the bytes the operation has to move (the blob read plus the blob
written: a snapshot reads the pool's arrays and writes the blob, a restore the other way round, a fork both), bytes
over time, and that rate as a share of the HBM peak (8.0 TB/s; a plain copy kernel reaches 6.3 TB/s).  The last line
sets the whole-pool `snapshot_device(rng=False)` + `restore_device` pair -- wall time, host clock around calls that
end in a stream synchronise -- against `get_state` + `set_state`, which move the same state through host memory.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # MI355X HBM3E, bytes/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("task")
    ap.add_argument("num_envs", type=int)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--roll", type=int, default=8)
    args = ap.parse_args()
    import torch

    import envpool_amd as envpool
    from envpool_amd import torch_interop as ti

    n = args.num_envs
    env = envpool.make(args.task, env_type="gymnasium", num_envs=n, seed=0)
    pool = env.device_pool
    dev = torch.device("cuda", pool.device)
    stream = torch.cuda.ExternalStream(pool.stream, device=dev)
    rng = np.random.default_rng(0)
    space = env.action_space
    env.reset()
    for _ in range(args.roll):
        if hasattr(space, "n"):
            act = rng.integers(0, space.n, n).astype(pool.action_dtype)
        else:
            act = rng.uniform(space.low, space.high, (n, *space.shape)).astype(pool.action_dtype)
        env.step(act)
    ids = np.arange(n, dtype=np.int32)
    src = np.roll(ids, 1)  # fork: every env becomes its neighbour

    def events(fn):
        """Median ms between two events on the pool's stream around one call."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for r in range(args.warmup + args.reps):
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            if r >= args.warmup:
                ms.append(a.elapsed_time(b))
        return float(np.median(ms))

    def wall(fn):
        """Median ms of a call that ends synchronised, by the host clock."""
        ms = []
        for r in range(args.warmup + args.reps):
            pool.synchronize()
            t0 = time.perf_counter()
            fn()
            pool.synchronize()
            if r >= args.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms))

    def line(op, ms, nbytes, **more):
        rate = nbytes / (ms * 1e-3)
        print(json.dumps({"task": args.task, "num_envs": n, "op": op, "ms": round(ms, 4), "bytes_moved": nbytes,
                          "gb_per_s": round(rate / 1e9, 1), "hbm_peak_fraction": round(rate / HBM_PEAK, 4), **more}),
              flush=True)

    pair_ms = {}
    for use_rng in (True, False):
        nbytes = pool.snapshot_bytes(n, use_rng)
        blob = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        blob = ti.snapshot_device(pool, out=blob, rng=use_rng)
        tag = "rng" if use_rng else "no_rng"
        line(f"snapshot_device[{tag}]", events(lambda: ti.snapshot_device(pool, out=blob, rng=use_rng)), 2 * nbytes)
        line(f"restore_device[{tag}]", events(lambda: ti.restore_device(pool, blob)), 2 * nbytes)
        line(f"fork[{tag}]", events(lambda: ti.fork(pool, src, ids, rng=use_rng)), 4 * nbytes)
        ti.restore_device(pool, blob)  # (the fork rotated the envs)

        def pair():
            ti.restore_device(pool, ti.snapshot_device(pool, out=blob, rng=use_rng))

        pair_ms[tag] = wall(pair)
    state_bytes = 8 * n * pool.state_dim()
    get_ms = wall(lambda: pool.get_state(ids))
    state = pool.get_state(ids)
    set_ms = wall(lambda: pool.set_state(state, ids))
    both_ms = wall(lambda: pool.set_state(pool.get_state(ids), ids))
    line("get_state", get_ms, 2 * state_bytes)
    line("set_state", set_ms, 2 * state_bytes)
    print(json.dumps({"task": args.task, "num_envs": n, "op": "pair",
                      "snapshot_restore_device_no_rng_wall_ms": round(pair_ms["no_rng"], 4),
                      "snapshot_restore_device_rng_wall_ms": round(pair_ms["rng"], 4),
                      "get_state_set_state_wall_ms": round(both_ms, 4),
                      "device_pair_is_faster": bool(pair_ms["no_rng"] < both_ms)}), flush=True)
    env.close()


if __name__ == "__main__":
    main()
