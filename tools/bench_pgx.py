"""PGX board-game env-steps/s on one MI355X: TicTacToe-v1, ConnectFour-v1, Hex-v1 and Othello-v1 at N = 65536 and
N = 1 << 20, on the device path (step_device, actions resident in HBM) and on the numpy path (send / recv of host
arrays).  The actions stay legal, so the numbers measure play and not resets after illegal moves: every step's
action is `(legal_action_mask * uniform).argmax` of the previous step's mask, drawn with torch on the GPU (device
path) or with numpy on the host (numpy path).  That masking is timed on its own too (`*_mask_ms_per_step`: the same
draw on a mask of the same size, without stepping) and is included in the `*_env_steps_per_s` figures.

Each line also gives the step kernels' achieved bytes/s (the device loop less its masking) against the HBM peak,
from a LOWER BOUND on the HBM bytes of one env-step:
  outputs      every state key's row, written (Hex: 968 B obs + 484 B board + 122 B mask + 45 B of the rest)
  action       4 B, read
  bookkeeping  done (1) and elapsed step (4) read + written, the generator position (4) read
  env state    the 64-byte pgx::State, read once and written once
Not counted: the generator words a reset draws (one) and cache-line granularity.

    python tools/bench_pgx.py [--steps 50] [--warmup 10] [--sizes 65536,1048576]
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
STATE_BYTES = 64
TASKS = ["TicTacToe-v1", "ConnectFour-v1", "Hex-v1", "Othello-v1"]
MASK_KEY = "info:legal_action_mask"


def algorithmic_bytes(pool):
    out = sum(int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize for _, dt, shape in pool.state_keys)
    return out + 4 + 2 * (1 + 4) + 4 + 2 * STATE_BYTES


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
    from envpool_amd.torch_interop import _DevArray

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    for task in args.tasks.split(","):
        native = type(envpool_amd.make_spec(task)).__name__[:-len("EnvSpec")]
        for n in [int(s) for s in args.sizes.split(",")]:
            pool = DevicePool(native, n, seed=0)
            mk = [k for k, _, _ in pool.state_keys].index(MASK_KEY)
            _, _, mshape = pool.state_keys[mk]
            ids = np.arange(n, dtype=np.int32)
            views = {}

            def mask_of(ptrs):
                t = views.get(ptrs[mk])
                if t is None:
                    t = views[ptrs[mk]] = torch.as_tensor(_DevArray(ptrs[mk], (n, *mshape), np.bool_), device=dev)
                return t

            def legal(mask):
                return (mask.float() * torch.rand(mask.shape, device=dev, generator=gen)).argmax(1).to(torch.int32)

            # device path
            pool.reset(ids)
            act = torch.as_tensor(pool.recv_dict()[MASK_KEY], device=dev)
            act = legal(act)
            for t in range(args.warmup + args.steps):
                if t == args.warmup:
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                pool.wait_stream(stream.cuda_stream)
                ptrs, _ = pool.step_device(act.data_ptr(), n)
                pool.consumer_wait(stream.cuda_stream)
                act = legal(mask_of(ptrs))
            torch.cuda.synchronize(dev)
            dev_s = time.perf_counter() - t0
            dev_rate = n * args.steps / dev_s
            mask = mask_of(ptrs).clone()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                act = legal(mask)
            torch.cuda.synchronize(dev)
            dev_mask_ms = (time.perf_counter() - t0) / args.steps * 1e3
            # numpy path
            rng = np.random.default_rng(0)
            pool.reset(ids)
            m = pool.recv_dict()[MASK_KEY]
            for t in range(args.warmup + args.steps):
                if t == args.warmup:
                    t0 = time.perf_counter()
                a = (m * rng.random(m.shape, dtype=np.float32)).argmax(1).astype(np.int32)
                pool.send(ids, a)
                m = pool.recv_dict()[MASK_KEY]
            np_rate = n * args.steps / (time.perf_counter() - t0)
            m = np.array(m)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                a = (m * rng.random(m.shape, dtype=np.float32)).argmax(1).astype(np.int32)
            np_mask_ms = (time.perf_counter() - t0) / args.steps * 1e3
            b = algorithmic_bytes(pool)
            # the step kernels alone: the loop's time less the masking (which runs on the same GPU between steps)
            dev_step_rate = n * args.steps / max(dev_s - args.steps * dev_mask_ms * 1e-3, 1e-9)
            print(json.dumps({"task": task, "num_envs": n, "device_env_steps_per_s": round(dev_rate),
                              "device_mask_ms_per_step": round(dev_mask_ms, 4),
                              "device_env_steps_per_s_less_mask": round(dev_step_rate),
                              "numpy_env_steps_per_s": round(np_rate),
                              "numpy_mask_ms_per_step": round(np_mask_ms, 3),
                              "bytes_per_env_step_lower_bound": b, "device_bytes_per_s": round(dev_step_rate * b),
                              "hbm_fraction_lower_bound": round(dev_step_rate * b / HBM_PEAK, 4)}),
                  flush=True)
            pool.close()


if __name__ == "__main__":
    main()
