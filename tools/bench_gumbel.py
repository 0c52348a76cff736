"""Gumbel search of the PGX games on one MI355X: the time of one `advance` launch in the device form and the roots x
simulations per second of whole sessions, with a constant evaluator so that the kernels are timed and not a model.
The PUCT figures to set beside it come from `tools/bench_guided.py` run in the same session on the same machine.

    python tools/bench_gumbel.py [--games Othello,Hex] [--sizes 4096] [--reps 5] [--warmup 1] [--out FILE]

Per game and k freshly reset roots, S = 32 simulations, m = 16 considered actions, one JSON line:
  advance   after `warmup` whole sessions, `reps` sessions; every one of a session's S + 1 `gumbel_advance_device`
            launches sits between its own pair of events on the pool's stream; the median over all of them, and the
            median of the launches t = S/2 .. S-1 alone (deep trees).  The logits (0 everywhere), the values (0) and
            the noise (a seeded draw) are three tensors made once: no evaluator runs between the launches.
  session   one pair of events around a session's begin and all its advances; the median over the sessions, and
            roots x simulations per second = k * S / median
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, M = 32, 16


def measure(torch, ti, DevicePool, fam, k, args):
    pool = DevicePool(fam, k, seed=0)
    dev = torch.device("cuda", pool.device)
    stream = torch.cuda.ExternalStream(pool.stream, device=dev)
    ids = torch.arange(k, dtype=torch.int32, device=dev)
    ti.send_device_tensors(pool, None, ids)  # reset: every env at the start of a game
    ti.recv_device_tensors(pool)
    h, w, c, a = pool.guided_shape()
    obs = torch.empty((k, h, w, c), dtype=torch.bool, device=dev)
    mask = torch.empty((k, a), dtype=torch.bool, device=dev)
    status = torch.empty((k,), dtype=torch.uint8, device=dev)
    noise = np.random.Generator(np.random.PCG64(0)).gumbel(size=(k, a)).astype(np.float32)
    gumbel = torch.from_numpy(noise).to(dev)
    logits = torch.zeros((k, a), dtype=torch.float32, device=dev)
    values = torch.zeros((k,), dtype=torch.float32, device=dev)
    visits = torch.empty((k, a), dtype=torch.int32, device=dev)
    vals = torch.empty((k, a), dtype=torch.float32, device=dev)
    action = torch.empty((k,), dtype=torch.int32, device=dev)
    weights = torch.empty((k, a), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    launches, deep, sessions = [], [], []
    for rep in range(args.warmup + args.reps):
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(S + 3)]
        evs[0].record(stream)
        pool.gumbel_begin_device(gumbel.data_ptr(), obs.data_ptr(), mask.data_ptr(), status.data_ptr(), None, S, M)
        evs[1].record(stream)
        for t in range(S + 1):
            pool.gumbel_advance_device(logits.data_ptr(), values.data_ptr(), k, obs.data_ptr(), mask.data_ptr(),
                                       status.data_ptr())
            evs[t + 2].record(stream)
        pool.gumbel_result_device(visits.data_ptr(), vals.data_ptr(), action.data_ptr(), weights.data_ptr())
        evs[-1].synchronize()
        torch.cuda.synchronize(dev)
        if rep >= args.warmup:
            ms = [evs[t + 1].elapsed_time(evs[t + 2]) for t in range(S + 1)]
            launches += ms
            deep += ms[S // 2:S]
            sessions.append(evs[0].elapsed_time(evs[-1]))
    assert bool((visits.sum(1) == S).all()) and bool((status == 2).all())
    assert bool(((weights.sum(1) - 1).abs() < 1e-5).all()) and bool((action >= 0).all())
    pool.guided_end()
    pool.close()
    session_ms = float(np.median(sessions))
    return {"game": fam, "roots": k, "simulations": S, "max_considered": M,
            "advance_us_per_launch": round(float(np.median(launches)) * 1e3, 2),
            "advance_us_per_launch_deep": round(float(np.median(deep)) * 1e3, 2),
            "advance_us_min_max": [round(min(launches) * 1e3, 2), round(max(launches) * 1e3, 2)],
            "session_ms": round(session_ms, 3), "session_ms_all": [round(x, 3) for x in sessions],
            "roots_simulations_per_s": float(k * S / (session_ms * 1e-3))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", default="Othello,Hex")
    ap.add_argument("--sizes", default="4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from envpool_amd import torch_interop as ti
    from envpool_amd.core.device_pool import DevicePool

    sink = open(args.out, "w") if args.out else None
    for fam in args.games.split(","):
        for k in [int(x) for x in args.sizes.split(",")]:
            text = json.dumps(measure(torch, ti, DevicePool, fam, k, args))
            print(text, flush=True)
            if sink:
                sink.write(text + "\n")
                sink.flush()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
