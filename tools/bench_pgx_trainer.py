"""A training step of the built-in nets: `tr.step` of the PGX trainer (csrc/pgx_trainer.hip) beside the README's loop
on the same net and rows -- `module(kernels=True)`, the torch loss, `torch.optim.SGD` with momentum, `zero_grad` --,
both on resident device tensors.  The protocol of tools/bench_pgx_train.py: alternating windows, the median and the
spread (min .. max) of the windows' ms per step.

    python tools/bench_pgx_trainer.py [--windows 7] [--steps 20]
"""
import argparse
import time

import numpy as np
import torch

from envpool_amd.pgx.net import ConvNet, Net


def torch_step(m, opt, obs, mask, pi, z):
    opt.zero_grad()
    logits, value = m(obs)
    logp = torch.log_softmax(logits.double().masked_fill(~mask, -1e30), dim=1)
    loss = -(pi * logp.masked_fill(~mask, 0.0)).sum(1).mean() + ((value.double() - z) ** 2).mean()
    loss.backward()
    opt.step()


def window(fn, steps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cases = [("Net D128 L2", lambda: Net.random((8, 8, 2), 65, 128, 2, seed=0), (4096, 65536)),
             ("Net D512 L4", lambda: Net.random((8, 8, 2), 65, 512, 4, seed=0), (4096, 65536)),
             ("ConvNet D64 L4 P4", lambda: ConvNet.random((8, 8, 2), 65, 64, 4, 4, seed=0), (4096,))]
    for name, make, sizes in cases:
        for rows in sizes:
            net = make()
            rng = np.random.default_rng(1)
            obs = torch.tensor((rng.random((rows, 128)) < 0.25).astype(np.uint8), device=dev)
            mask = torch.tensor(rng.random((rows, 65)) < 0.5, device=dev)
            mask[:, 0] = True
            pi = torch.tensor(rng.random((rows, 65)).astype(np.float32), device=dev) * mask
            pi = pi / pi.sum(1, keepdim=True)
            z = torch.tensor(rng.uniform(-1, 1, rows).astype(np.float32), device=dev)
            tr = net.trainer(lr=1e-3, momentum=0.9, max_rows=rows)
            m = net.module(kernels=True).to(dev)
            opt = torch.optim.SGD(m.parameters(), lr=1e-3, momentum=0.9)
            mask8, obs_f = mask.view(torch.uint8), obs.double()
            ours = lambda: tr.step(obs, mask8, pi, z)
            theirs = lambda: torch_step(m, opt, obs_f, mask, pi, z)
            window(ours, 3), window(theirs, 3)
            t = [[], []]
            for _ in range(a.windows):
                t[0].append(window(ours, a.steps))
                t[1].append(window(theirs, a.steps))
            f = lambda x: f"{np.median(x):.3f} ms ({min(x):.3f} .. {max(x):.3f})"
            print(f"{name} rows {rows}: trainer {f(t[0])}; torch loop {f(t[1])}; "
                  f"ratio {np.median(t[1]) / np.median(t[0]):.2f}", flush=True)
            tr.close()


if __name__ == "__main__":
    main()
