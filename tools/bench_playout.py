"""Random playouts of the PGX games on one MI355X: the fused playout kernel (device form) beside the loop a caller has
to write without it, both from freshly reset positions to the end of every game.

    python tools/bench_playout.py [--games TicTacToe,ConnectFour,Hex,Othello] [--reps 300] [--warmup 3] [--out FILE]

Per game and shape -- N = 65536 envs x R = 1 repeat, and N = 8192 x R = 8 -- one JSON line:
  playout   `torch_interop.playout_device`, timed with events on the pool's stream around `reps` launches (a new seed
            for each), plies per second = plies played in those launches / that time
  loop      `send_device_tensors` / `recv_device_tensors` of a pool of N x R envs with the action picked uniformly from
            `info:legal_action_mask` in torch, until every env's first game is over (the host looks every 4 steps); only
            the plies of those first games count; host clock around a loop that ends in a device synchronise.  The same
            pool serves both shapes: without the kernel R repeats of a position are R envs.
  wave efficiency   sum(plies) / (64 * sum over waves of the wave's longest playout), from the returned plies and the
            lane mapping (lane = env row * R + repeat, 64 consecutive lanes a wave): the share of lane-plies that are
            not idle waiting for the wave's longest game
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(65536, 1), (8192, 8)]


def wave_efficiency(plies):
    lanes = np.asarray(plies, np.int64).reshape(-1)
    pad = (-len(lanes)) % 64
    waves = np.concatenate([lanes, np.zeros(pad, np.int64)]).reshape(-1, 64)
    return float(lanes.sum() / max(64 * waves.max(axis=1).sum(), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", default="TicTacToe,ConnectFour,Hex,Othello")
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from envpool_amd import torch_interop as ti
    from envpool_amd.core.device_pool import DevicePool

    sink = open(args.out, "w") if args.out else None

    def emit(rec):
        text = json.dumps(rec)
        print(text, flush=True)
        if sink:
            sink.write(text + "\n")
            sink.flush()

    for fam in args.games.split(","):
        loop_rate = None
        for n, r in SHAPES:
            pool = DevicePool(fam, n, seed=0)
            dev = torch.device("cuda", pool.device)
            stream = torch.cuda.ExternalStream(pool.stream, device=dev)
            ids = torch.arange(n, dtype=torch.int32, device=dev)
            ti.send_device_tensors(pool, None, ids)  # reset: every env at the start of a game
            ti.recv_device_tensors(pool)
            for w in range(args.warmup):
                ti.playout_device(pool, None, repeats=r, seed=1000 + w)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            plies_dev, status_dev = [], []
            torch.cuda.synchronize(dev)
            a.record(stream)
            for i in range(args.reps):
                _, p, st = ti.playout_device(pool, None, repeats=r, seed=i)
                plies_dev.append(p)
                status_dev.append(st)
            b.record(stream)
            b.synchronize()
            ms = a.elapsed_time(b)
            assert not bool(torch.stack(status_dev).any())  # every game was played to its end
            total = int(torch.stack(plies_dev).sum(dtype=torch.int64))
            plies = np.stack([p.cpu().numpy() for p in plies_dev[:10]])  # the statistics: the first ten launches
            rec = {"game": fam, "num_envs": n, "repeats": r, "launches": args.reps,
                   "playout_ms_per_launch": round(ms / args.reps, 4),
                   "playout_plies_per_s": float(total / (ms * 1e-3)),
                   "plies_mean": round(float(plies.mean()), 2), "plies_max": int(plies.max()),
                   "wave_efficiency": round(float(np.mean([wave_efficiency(p) for p in plies])), 4)}
            pool.close()
            if loop_rate is None:
                loop_rate = step_loop(torch, ti, DevicePool, fam, n * r, args)
            rec.update(loop_rate)
            rec["playout_over_loop"] = round(rec["playout_plies_per_s"] / rec["loop_plies_per_s"], 2)
            emit(rec)
    if sink:
        sink.close()


def step_loop(torch, ti, DevicePool, fam, n, args):
    """The caller's loop on a pool of n envs: plies per second of the envs' first games."""
    pool = DevicePool(fam, n, seed=0)
    dev = torch.device("cuda", pool.device)
    ids = torch.arange(n, dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    rates, steps_seen = [], 0
    for rep in range(4):  # the first one warms up
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        ti.send_device_tensors(pool, None, ids)
        out = ti.recv_device_tensors(pool)
        alive = torch.ones(n, dtype=torch.bool, device=dev)
        played = torch.zeros((), dtype=torch.int64, device=dev)
        steps = 0
        while True:
            mask = out["info:legal_action_mask"]
            act = (mask.float() * torch.rand(mask.shape, device=dev, generator=gen)).argmax(1).to(torch.int32)
            ti.send_device_tensors(pool, act, ids)
            out = ti.recv_device_tensors(pool)
            played += alive.sum()
            alive &= ~out["done"].bool()
            steps += 1
            if steps % 4 == 0 and not bool(alive.any()):
                break
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        if rep > 0:
            rates.append(float(played.item()) / dt)
            steps_seen = steps
    pool.close()
    return {"loop_envs": n, "loop_steps": steps_seen, "loop_plies_per_s": float(np.median(rates))}


if __name__ == "__main__":
    main()
