"""MiniGrid env-steps/s on one MI355X: DoorKey-8x8, FourRooms and Dynamic-Obstacles-8x8 at N = 65536 and
N = 1 << 20, on the device path (actions resident in HBM, step_device: send + recv in one call, no PCIe)
and on the numpy path (send / recv of host arrays).  Each line also gives the device path's achieved bytes/s
against the HBM peak, from a LOWER BOUND on the HBM bytes of one env-step computed here:
  outputs    every state key's row (289 B: the 147 B image and 96 B mission of them), written
  action     4 B read
  env state  agent word (4), carried word (2), done (1), step count (4), generator position (4), and for
             Dynamic-Obstacles the obstacle word (8): read + written
  view       the 7 x 7 window of 2-byte cells, read
  generator  Dynamic-Obstacles only: at least 2 draws per obstacle per step; the tiled mt19937 regenerates one
             16-word tile per 16 draws (own tile 64 B read + written, 16 partner words read: 192 B), i.e.
             12 B per draw
Not counted: resets (they write the whole grid and draw more, at a rate the tool does not know), rejected
obstacle moves (more draws), and cache-line granularity of the scattered accesses.  So `hbm_fraction_lower_bound`
is what it says.

    python tools/bench_minigrid.py [--steps 50] [--warmup 10]
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
TASKS = ["MiniGrid-DoorKey-8x8-v0", "MiniGrid-FourRooms-v0", "MiniGrid-Dynamic-Obstacles-8x8-v0"]


def algorithmic_bytes(pool, n_obstacles):
    out = sum(int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize for _, dt, shape in pool.state_keys)
    state = 2 * (4 + 2 + 1 + 4 + 4 + (8 if n_obstacles else 0))
    draws = 2 * n_obstacles
    return out + 4 + state + 49 * 2 + 12 * draws


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sizes", default="65536,1048576")
    args = ap.parse_args()
    import torch

    import envpool_amd
    from envpool_amd.core.device_pool import DevicePool
    from envpool_amd.minigrid import _native_params

    dev = torch.device("cuda", 0)
    for task in TASKS:
        conf = envpool_amd.make_spec(task).config._asdict()
        p = {k: float(v) for k, v in _native_params(conf).items()}
        n_obst = 0
        if conf["env_name"] == "dynamic_obstacles":  # DynamicObstaclesTask's clamp
            n_obst = conf["n_obstacles"] if conf["n_obstacles"] <= conf["size"] // 2 + 1 else conf["size"] // 2
        hi = conf["action_max"] + 1
        for n in [int(s) for s in args.sizes.split(",")]:
            pool = DevicePool("MiniGrid", n, seed=0, max_episode_steps=conf["max_episode_steps"], params=p)
            ids = np.arange(n, dtype=np.int32)
            acts = torch.randint(0, hi, (args.warmup + args.steps, n), dtype=torch.int32, device=dev)
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
            b = algorithmic_bytes(pool, n_obst)
            print(json.dumps({"task": task, "num_envs": n, "device_env_steps_per_s": round(dev_rate),
                              "numpy_env_steps_per_s": round(np_rate), "bytes_per_env_step_lower_bound": b,
                              "device_bytes_per_s": round(dev_rate * b),
                              "hbm_fraction_lower_bound": round(dev_rate * b / HBM_PEAK, 4)}),
                  flush=True)
            pool.close()


if __name__ == "__main__":
    main()
