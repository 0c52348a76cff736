"""Rollout collector against the same bookkeeping done with torch, on the device path, actions already on the device.

For HalfCheetah-v4 and CartPole-v1 at num_envs = 65536 and a horizon of T = 32 it times one horizon
  collector   T x rollout_step_device (env step + the collector's kernels), rollout_gae_device, rollout_next
  torch       T x send_device_tensors / recv_device_tensors plus index-copies of obs, action, reward and the flags into
              preallocated [T(+1), N, ...] tensors by env id, the mask from the carried done flag, and a GAE loop over T
              in torch (selects, float32)
and prints one JSON line per env: env-steps/s of both (median of `--repeats` windows of `--horizons` horizons each, the
two paths alternating, every window ending in a device synchronise) and their spread.  `--check` compares the two
paths' buffers and advantages once.  `--collector-only` runs the collector windows alone: the run to put under a
kernel trace for the device time of each collector kernel (RolloutStore, RolloutScan, RolloutGae, RolloutMoments,
RolloutMomentsFold)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import envpool_amd as envpool  # noqa: E402
from envpool_amd import torch_interop as ti  # noqa: E402


def make_pool(task, n, seed):
    env = envpool.make(task, "gymnasium", num_envs=n, seed=seed)
    return env, env.device_pool


def action_bank(env, pool, horizon, dev, seed):
    rng = np.random.default_rng(seed)
    shape = (horizon, pool.num_envs, *pool.action_shape)
    if hasattr(env.action_space, "n"):
        a = rng.integers(0, env.action_space.n, shape).astype(pool.action_dtype)
    else:
        a = rng.uniform(env.action_space.low, env.action_space.high, shape).astype(pool.action_dtype)
    return torch.from_numpy(a).to(dev)


class Collector:
    def __init__(self, task, n, horizon, seed, moments):
        self.env, self.pool = make_pool(task, n, seed)
        self.dev = torch.device("cuda", self.pool.device)
        self.T = horizon
        self.pool.rollout_begin(horizon, 1 << 16, moments)
        self.actions = action_bank(self.env, self.pool, horizon, self.dev, seed)
        self.out = (torch.empty((horizon, n), dtype=torch.float32, device=self.dev),
                    torch.empty((horizon, n), dtype=torch.float32, device=self.dev))
        ti.rollout_reset_device(self.pool)

    def horizon(self, values):
        for t in range(self.T):
            ti.rollout_step_device(self.pool, self.actions[t])
        ti.rollout_gae_device(self.pool, values, 0.99, 0.95, out=self.out)
        self.pool.rollout_next()

    def result(self):
        v = ti.rollout_view_device(self.pool)
        return v, self.out


class TorchLoop:
    """The parent commit's calls: the pool's device path and torch for everything else."""

    def __init__(self, task, n, horizon, seed):
        self.env, self.pool = make_pool(task, n, seed)
        self.dev = dev = torch.device("cuda", self.pool.device)
        self.T, self.n = horizon, n
        self.actions = action_bank(self.env, self.pool, horizon, dev, seed)
        ti.send_device_tensors(self.pool, None)
        out = ti.recv_device_tensors(self.pool)
        obs = out["obs"]
        self.obs = torch.zeros((horizon + 1, *obs.shape), dtype=obs.dtype, device=dev)
        self.action = torch.zeros_like(self.actions)
        self.reward = torch.zeros((horizon, n), dtype=torch.float32, device=dev)
        self.term = torch.zeros((horizon, n), dtype=torch.bool, device=dev)
        self.trunc = torch.zeros((horizon, n), dtype=torch.bool, device=dev)
        self.mask = torch.zeros((horizon, n), dtype=torch.bool, device=dev)
        self.carry = torch.zeros(n, dtype=torch.bool, device=dev)
        self.adv = torch.zeros((horizon, n), dtype=torch.float32, device=dev)
        self.ret = torch.zeros((horizon, n), dtype=torch.float32, device=dev)
        self.obs[0].index_copy_(0, out["info:env_id"].long(), obs)

    def horizon(self, values):
        for t in range(self.T):
            ti.send_device_tensors(self.pool, self.actions[t])
            out = ti.recv_device_tensors(self.pool)
            idx = out["info:env_id"].long()
            done, trunc = out["done"], out["trunc"]
            self.obs[t + 1].index_copy_(0, idx, out["obs"])
            self.action[t].index_copy_(0, idx, self.actions[t])
            self.reward[t].index_copy_(0, idx, out["reward"].reshape(-1))
            self.term[t].index_copy_(0, idx, done & ~trunc)
            self.trunc[t].index_copy_(0, idx, trunc)
            self.mask[t] = ~self.carry
            self.carry.index_copy_(0, idx, done)
        gamma, gl = 0.99, float(np.float32(np.float32(0.99) * np.float32(0.95)))
        nxt = torch.zeros(self.n, dtype=torch.float32, device=self.dev)
        zero = torch.zeros((), dtype=torch.float32, device=self.dev)
        for t in range(self.T - 1, -1, -1):
            d = torch.where(self.term[t], self.reward[t], self.reward[t] + gamma * values[t + 1])
            delta = d - values[t]
            a = torch.where(self.term[t] | self.trunc[t], delta, delta + gl * nxt)
            a = torch.where(self.mask[t], a, zero)
            self.adv[t], self.ret[t], nxt = a, a + values[t], a
        self.obs[0].copy_(self.obs[self.T])


def window(path, values, horizons, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(horizons):
        path.horizon(values)
    torch.cuda.synchronize(dev)
    path.pool.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--horizons", type=int, default=8, help="horizons per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2, help="warm-up horizons per path")
    ap.add_argument("--tasks", default="HalfCheetah-v4,CartPole-v1")
    ap.add_argument("--moments", action="store_true", help="the collector also keeps observation moments")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--collector-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout: no GPU; there is nothing to measure without one")
    for task in args.tasks.split(","):
        n, T = args.num_envs, args.horizon
        col = Collector(task, n, T, 1, args.moments)
        dev = col.dev
        values = torch.from_numpy(np.random.default_rng(2).normal(0, 1, (T + 1, n)).astype(np.float32)).to(dev)
        base = None if args.collector_only else TorchLoop(task, n, T, 1)
        if args.check and base is not None:
            col.horizon(values)
            base.horizon(values)
            torch.cuda.synchronize(dev)
            v, (adv, ret) = col.result()
            same = {"obs": torch.equal(v["obs"][1:], base.obs[1:]), "reward": torch.equal(v["reward"], base.reward),
                    "mask": torch.equal(v["mask"].bool(), base.mask), "term": torch.equal(v["term"].bool(), base.term),
                    "adv_max_abs_diff": float((adv - base.adv).abs().max())}
            print(json.dumps({"task": task, "check": same}))
        for _ in range(args.warmup):
            col.horizon(values)
            if base is not None:
                base.horizon(values)
        tc, tb = [], []
        for _ in range(args.repeats):
            tc.append(window(col, values, args.horizons, dev))
            if base is not None:
                tb.append(window(base, values, args.horizons, dev))
        steps = args.horizons * T * n

        def rate(ts):
            return {"median": steps / float(np.median(ts)), "min": steps / max(ts), "max": steps / min(ts)}

        line = {"task": task, "num_envs": n, "horizon": T, "moments": args.moments, "unit": "env-steps/s",
                "collector": rate(tc)}
        if base is not None:
            line["torch_loop"] = rate(tb)
            line["collector_over_torch_loop"] = line["collector"]["median"] / line["torch_loop"]["median"]
        print(json.dumps(line), flush=True)
        col.pool.rollout_end()


if __name__ == "__main__":
    main()
