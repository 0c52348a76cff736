"""The masked head of the rollout actor (kind 2) beside a discrete actor (kind 0) of the same net on the same Game2048
pool: one `collect()` of a horizon, and one `fit` of it, in the same process, legs alternating.  HIP events on torch's
stream around calls that only enqueue (both are ordered against the pool's stream both ways); a warm-up, then the median
and the spread (min .. max) of the repeats.

    python tools/bench_actor_masked.py [--repeats 9] [--envs 65536] [--horizon 32] [--batch 4096] [--epochs 4]
"""
import argparse

import numpy as np
import torch

import envpool_amd as envpool
from envpool_amd import torch_interop as ti
from envpool_amd.actor import Actor


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--epochs", type=int, default=4)
    a = ap.parse_args()
    torch.cuda.init()
    env = envpool.make("Game2048-v1", "gymnasium", num_envs=a.envs, seed=1)
    ro = env.rollout(horizon=a.horizon)
    pool = env._rollout()
    masked = Actor.random(env, hidden=64, blocks=1, seed=0, mask=True)
    plain = Actor(masked.net, 0, masked.lo, masked.scale)
    legs = {"masked (kind 2)": masked, "discrete (kind 0)": plain}
    batch = min(a.batch, a.envs * a.horizon)
    trainers = {k: v.trainer(lr=1e-3, max_rows=batch) for k, v in legs.items()}
    ro.attach(masked, seed=1)
    ro.reset()
    collect = {k: [] for k in legs}
    fit = {k: [] for k in legs}
    for rep in range(a.repeats + 1):  # (the first repeat is the warm-up)
        for name, actor in legs.items():
            ro.attach(actor, seed=1)
            c = timed(lambda: ti.rollout_collect_device(pool))
            f = timed(lambda: trainers[name].fit(ro, epochs=a.epochs, batch=batch))
            ro.next()
            if rep:
                collect[name].append(c)
                fit[name].append(f)
    show = lambda x: f"{np.median(x):.3f} ms ({min(x):.3f} .. {max(x):.3f})"
    for name in legs:
        print(f"Game2048-v1 T {a.horizon} N {a.envs} {name}: collect {show(collect[name])}; fit of {a.epochs} epochs, "
              f"batch {batch}: {show(fit[name])}", flush=True)
    for t in trainers.values():
        t.close()
    ro.close()


if __name__ == "__main__":
    main()
