"""Jumanji board-puzzle env-steps/s on one MI355X: every registered id at N = 65536 and N = 1 << 20, on the
device path (actions resident in HBM, step_device: send + recv in one call, no PCIe) and on the numpy path
(send / recv of host arrays).  Each line also gives the device path's achieved bytes/s against the HBM peak,
from a LOWER BOUND on the HBM bytes of one env-step computed here:
  outputs    every state key's row, written (Snake: 2880 B of obs:grid of its 2904)
  action     4 B per action element, read
  bookkeeping done (1) and elapsed step (4) read + written, the generator position (4) read
  env state  the per-env state struct (csrc/jumanji_env.hip.h: 64 / 200 / 108 / 56 / 160 / 104 B), read once:
             every observation reports the whole board
Not counted: state bytes written back, generator words (a reset draws 2 .. 400 of them, a step 0 .. 3), and
cache-line granularity.  So `hbm_fraction_lower_bound` is what it says.

    python tools/bench_jumanji.py [--steps 50] [--warmup 10] [--sizes 65536,1048576]
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
STATE_BYTES = {"Game2048": 64, "Minesweeper": 200, "SlidingTilePuzzle": 108, "RubiksCube": 56, "Snake": 160,
               "Maze": 104}
TASKS = ["Game2048-v1", "Minesweeper-v0", "SlidingTilePuzzle-v0", "RubiksCube-v0", "RubiksCube-partly-scrambled-v0",
         "Snake-v1", "Maze-v0"]


def algorithmic_bytes(pool, native):
    out = sum(int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize for _, dt, shape in pool.state_keys)
    act = 4 * int(np.prod(pool.action_shape, dtype=np.int64))
    return out + act + 2 * (1 + 4) + 4 + STATE_BYTES[native]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--tasks", default=",".join(TASKS))
    args = ap.parse_args()
    import torch

    import envpool_amd
    from envpool_amd.core.device_pool import DevicePool
    from envpool_amd.jumanji import FAMILIES

    dev = torch.device("cuda", 0)
    for task in args.tasks.split(","):
        spec = envpool_amd.make_spec(task)
        conf = spec.config._asdict()
        fd = FAMILIES[type(spec).__name__[:-len("EnvSpec")]]
        p = {k: float(v) for k, v in fd.native_params(conf).items()}
        for n in [int(s) for s in args.sizes.split(",")]:
            pool = DevicePool(fd.native, n, seed=0, max_episode_steps=conf["max_episode_steps"], params=p)
            ids = np.arange(n, dtype=np.int32)
            shape = tuple(pool.action_shape)
            acts = torch.randint(0, 4, (args.warmup + args.steps, n, *shape), dtype=torch.int32, device=dev)
            pool.reset(ids)
            pool.recv()
            for t in range(args.warmup):
                pool.step_device(acts[t].data_ptr(), n)
            pool.synchronize()
            t0 = time.perf_counter()
            for t in range(args.steps):
                pool.step_device(acts[args.warmup + t].data_ptr(), n)
            pool.synchronize()
            dev_rate = n * args.steps / (time.perf_counter() - t0)
            host_acts = acts.cpu().numpy()
            for t in range(args.warmup):
                pool.send(ids, host_acts[t])
                pool.recv()
            t0 = time.perf_counter()
            for t in range(args.steps):
                pool.send(ids, host_acts[args.warmup + t])
                pool.recv()
            np_rate = n * args.steps / (time.perf_counter() - t0)
            b = algorithmic_bytes(pool, fd.native)
            print(json.dumps({"task": task, "num_envs": n, "device_env_steps_per_s": round(dev_rate),
                              "numpy_env_steps_per_s": round(np_rate), "bytes_per_env_step_lower_bound": b,
                              "device_bytes_per_s": round(dev_rate * b),
                              "hbm_fraction_lower_bound": round(dev_rate * b / HBM_PEAK, 4)}),
                  flush=True)
            pool.close()


if __name__ == "__main__":
    main()
