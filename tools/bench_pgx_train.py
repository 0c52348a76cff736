"""Device time of one training step's forward + backward of the PGX built-in network on one MI355X: the training
kernels (`Net.module(kernels=True)`) beside (a) the float64 twin `Net.module()` on the same device and (b) a plain
torch MLP of the same shape under bf16 autocast, which is what a user would write instead.

    python tools/bench_pgx_train.py [--rows 4096,65536] [--reps 7] [--window-ms 30] [--out profiles/pgx_train_bench.txt]

Per setting -- an Othello net (F = 128, A = 65) at D = 128, L = 2 and at D = 512, L = 4 -- and row count one JSON line.
A step is `integers(x)` (the MLP: its forward), a loss in torch on p -- log-softmax cross-entropy over the A policy
columns plus the squared error of the value column -- and `backward()` down to every layer's weight and bias gradient;
no optimizer.  `*_us` is the device time between two events around `*_steps` back-to-back steps on torch's stream,
divided by that count: the median of `reps` windows taken in turns (kernels, twin, mlp, kernels, ..) after a warm-up of
each, with the spread (max - min) / median.  Every form gets as many steps per window as make it `--window-ms` long by
a pilot window, and at least 5, so that a window of the fast forms at few rows is tens of milliseconds too.  `gmacs` counts the multiply-accumulates of the three GEMMs per layer
(forward, dx, dW; no dx for the trunk), from the shapes."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = [(128, 65, 128, 2), (128, 65, 512, 4)]  # F, A, D, L


def macs_per_row(f, a, d, blocks):
    return 2 * f * d + 3 * (2 * blocks * d * d + (a + 1) * d)


def mlp(torch, f, a, d, blocks, dev):
    class Mlp(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.trunk = torch.nn.Linear(f, d)
            self.blocks = torch.nn.ModuleList(
                [torch.nn.ModuleList([torch.nn.Linear(d, d), torch.nn.Linear(d, d)]) for _ in range(blocks)])
            self.head = torch.nn.Linear(d, a + 1)

        def forward(self, x):
            h = torch.relu(self.trunk(x))
            for one, two in self.blocks:
                h = torch.relu(two(torch.relu(one(h))) + h)
            return self.head(h)

    return Mlp().to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="4096,65536")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    from envpool_amd.pgx.net import Net

    if not torch.cuda.is_available():
        raise SystemExit("bench_pgx_train: needs a GPU")
    dev = torch.device("cuda", 0)
    lines = []
    for f, a, d, blocks in SETTINGS:
        net = Net.random((8, 8, 2), a, d, blocks, seed=1)
        for rows in (int(r) for r in args.rows.split(",")):
            rng = np.random.default_rng(rows)
            x = torch.tensor((rng.random((rows, f)) < 0.25).astype(np.uint8), device=dev)
            target = torch.tensor(rng.integers(0, a, rows), device=dev)
            z = torch.tensor(rng.uniform(-1, 1, rows), device=dev)
            fast, twin, plain = net.module(kernels=True).to(dev), net.module().to(dev), mlp(torch, f, a, d, blocks, dev)
            x_half = x.to(torch.float32)

            def loss_of(p, scale_p, scale_v):
                logp = torch.log_softmax(p[:, :a] * scale_p, dim=1)
                return -logp.gather(1, target[:, None]).mean() + ((p[:, a] * scale_v - z) ** 2).mean()

            def step_net(m):
                m.zero_grad(set_to_none=True)
                loss_of(m.integers(x), net.scale_p, net.scale_v).backward()

            def step_mlp():
                plain.zero_grad(set_to_none=True)
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    p = plain(x_half)
                loss_of(p.float(), 1.0, 1.0).backward()

            forms = {"kernels": lambda: step_net(fast), "twin_f64": lambda: step_net(twin), "mlp_bf16": step_mlp}

            def window(step, steps):
                begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                begin.record()
                for _ in range(steps):
                    step()
                end.record()
                end.synchronize()
                return begin.elapsed_time(end) * 1e3 / steps

            for step in forms.values():  # warm-up: code objects, the handle, library algorithms
                step(), step()
            torch.cuda.synchronize()
            # the two net paths agree before they are timed
            got, want = [w.grad.clone() for w in fast.weights], [w.grad for w in twin.weights]
            worst = max(float(((g - w).abs().max() / w.abs().max()).cpu()) for g, w in zip(got, want))
            steps = {name: max(5, math.ceil(args.window_ms * 1e3 / window(step, 5))) for name, step in forms.items()}
            times = {name: [] for name in forms}
            for _ in range(args.reps):
                for name, step in forms.items():
                    times[name].append(window(step, steps[name]))
            line = {"F": f, "A": a, "D": d, "L": blocks, "rows": rows, "window_ms": args.window_ms,
                    "gmacs": round(rows * macs_per_row(f, a, d, blocks) / 1e9, 2),
                    "worst_grad_diff_over_max": float(f"{worst:.3g}")}
            for name, ts in times.items():
                med = statistics.median(ts)
                line[name + "_us"] = round(med, 1)
                line[name + "_steps"] = steps[name]
                line[name + "_spread"] = round((max(ts) - min(ts)) / med, 3)
            line["twin_over_kernels"] = round(line["twin_f64_us"] / line["kernels_us"], 2)
            line["mlp_over_kernels"] = round(line["mlp_bf16_us"] / line["kernels_us"], 2)
            print(json.dumps(line), flush=True)
            lines.append(json.dumps(line))
            del fast, twin, plain
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# tools/bench_pgx_train.py on one MI355X: device time of forward + loss + backward of one step, the "
                     "training kernels beside the float64 twin and a bf16-autocast torch MLP of the same shape\n")
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
