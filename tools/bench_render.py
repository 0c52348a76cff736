"""Render throughput on one MI355X: frames/s of the ten board games (six Jumanji puzzles, four PGX games) at each
game's default frame size for k = 4096 envs, through `torch_interop.render_device` (frames stay in HBM) and through
the host path `DevicePool.render` (frames copied into a numpy array), each with the render kernel's time from HIP
events around the launch.

The pool is first rolled `--roll` steps with random on-board actions, so the frames show boards in play (what a
frame costs depends on how many primitives the state puts on it).  Each line also gives the bytes one launch
writes (k * H * W * 3) and the share of the HBM peak they amount to over the kernel time.

    python tools/bench_render.py [--k 4096] [--reps 20] [--warmup 3] [--roll 8] [--games Game2048,Hex]
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
# game (the engine's family name) -> how many values a component of a random action takes
GAMES = {"Game2048": 4, "Minesweeper": 10, "SlidingTilePuzzle": 4, "RubiksCube": 3, "Snake": 4, "Maze": 4,
         "TicTacToe": 9, "ConnectFour": 7, "Hex": 121, "Othello": 64}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--roll", type=int, default=8)
    ap.add_argument("--games", default=",".join(GAMES))
    args = ap.parse_args()
    import torch

    from envpool_amd.core.device_pool import DevicePool
    from envpool_amd.torch_interop import render_device

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    k = args.k
    ids = np.arange(k, dtype=np.int32)
    for game in args.games.split(","):
        pool = DevicePool(game, k, seed=0)
        pool.reset(ids)
        pool.recv()
        for _ in range(args.roll):
            pool.send(ids, rng.integers(0, GAMES[game], (k, *pool.action_shape)).astype(pool.action_dtype))
            pool.recv()
        w, h = pool.render_size()
        nbytes = k * h * w * 3
        out = torch.empty((k, h, w, 3), dtype=torch.uint8, device=dev)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        kernel_ms = []
        for r in range(args.warmup + args.reps):
            if r == args.warmup:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
            start.record()
            render_device(pool, ids, out=out)
            end.record()
            if r >= args.warmup:
                end.synchronize()
                kernel_ms.append(start.elapsed_time(end))
        torch.cuda.synchronize(dev)
        dev_s = (time.perf_counter() - t0) / args.reps
        first = out[0].cpu().numpy()
        for r in range(2 + max(1, args.reps // 4)):
            if r == 2:
                t0 = time.perf_counter()
            frames = pool.render(ids)
        host_s = (time.perf_counter() - t0) / max(1, args.reps // 4)
        assert np.array_equal(frames[0], first)
        ms = float(np.median(kernel_ms))
        print(json.dumps({"game": game, "k": k, "width": w, "height": h, "bytes_per_launch": nbytes,
                          "kernel_ms": round(ms, 4), "kernel_frames_per_s": round(k / (ms * 1e-3)),
                          "hbm_write_fraction": round(nbytes / (ms * 1e-3) / HBM_PEAK, 4),
                          "device_frames_per_s": round(k / dev_s), "host_frames_per_s": round(k / host_s)}),
              flush=True)
        del out, frames
        pool.close()


if __name__ == "__main__":
    main()
