"""A PPO fit of a collected horizon: `tr.fit(ro, ...)` of the rollout actor's trainer (csrc/ppo_trainer.hip) beside the
README's loop on the same device and horizon -- the collector's GAE on the device, advantage normalisation, a torch
permutation per epoch, minibatch indexing in torch, `actor.module(kernels=True)`, the torch loss, `torch.optim.Adam`,
gradient clipping -- and, once per fit, `Actor.from_module`.  Actions, observations and everything else stay on the
device.  Alternating windows; the median and the spread (min .. max) of the windows' ms per fit.

    python tools/bench_ppo_trainer.py [--windows 5] [--fits 2] [--envs 65536] [--horizon 32]
"""
import argparse
import time

import numpy as np
import torch

import envpool_amd as envpool
from envpool_amd import torch_interop as ti
from envpool_amd.actor import Actor


def torch_fit(m, opt, pool, epochs, batch, out):
    view, (logp, value) = ti.rollout_view_device(pool), ti.actor_view_device(pool)
    adv, ret = ti.rollout_gae_device(pool, value, 0.99, 0.95, out=out)
    t, n = adv.shape
    obs = next(iter(view.values()))[:t].reshape((t * n, -1))
    act = view["action"].reshape((t * n,) + view["action"].shape[2:])
    mask = view["mask"].reshape(-1).bool()
    old, adv, ret = logp.reshape(-1), adv.reshape(-1), ret.reshape(-1)
    adv = (adv - adv[mask].mean()) / (adv[mask].std(unbiased=False) + 1e-8)
    for _ in range(epochs):
        perm = torch.randperm(t * n, device=obs.device)
        for s in range(t * n // batch):
            i = perm[s * batch:(s + 1) * batch]
            logits, v = m(obs[i].double())
            ratio = (m.logp_of(logits, act[i]) - old[i]).exp()
            a, w = adv[i], mask[i].double()
            policy = -(torch.min(ratio * a, ratio.clamp(0.8, 1.2) * a) * w).sum()
            loss = (policy + 0.5 * (((v - ret[i]) ** 2) * w).sum()) / batch
            opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(m.parameters(), 0.5)
            opt.step()
    actor = Actor.from_module(m.cpu())  # (the README's way back; the module returns to the device for the next fit)
    m.to(obs.device)
    return actor


def window(fn, fits):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(fits):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / fits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--fits", type=int, default=2)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=32)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.init()
    for task in ("CartPole-v1", "HalfCheetah-v4"):
        env = envpool.make(task, "gymnasium", num_envs=a.envs, seed=1)
        ro = env.rollout(horizon=a.horizon)
        actor = Actor.random(env, hidden=64, blocks=1, seed=0)
        ro.attach(actor, seed=1)
        ro.reset()
        ro.collect()
        pool = env._rollout()
        out = (torch.empty((a.horizon, a.envs), dtype=torch.float32, device=dev),
               torch.empty((a.horizon, a.envs), dtype=torch.float32, device=dev))
        for batch in (65536, 4096):
            batch = min(batch, a.envs * a.horizon)
            tr = actor.trainer(lr=1e-3, max_rows=batch)
            m = actor.module(kernels=True).to(dev)
            opt = torch.optim.Adam(m.parameters(), lr=1e-3)
            ours = lambda: tr.fit(ro, epochs=4, batch=batch)
            theirs = lambda: torch_fit(m, opt, pool, 4, batch, out)
            window(ours, 1), window(theirs, 1)
            t = [[], []]
            for _ in range(a.windows):
                t[0].append(window(ours, a.fits))
                t[1].append(window(theirs, a.fits))
            f = lambda x: f"{np.median(x):.2f} ms ({min(x):.2f} .. {max(x):.2f})"
            print(f"{task} T {a.horizon} N {a.envs} batch {batch}, 4 epochs: fit {f(t[0])}; torch loop {f(t[1])}; "
                  f"ratio {np.median(t[1]) / np.median(t[0]):.2f}", flush=True)
            tr.close()
        ro.close()


if __name__ == "__main__":
    main()
