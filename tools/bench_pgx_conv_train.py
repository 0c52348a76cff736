"""Device time of one training step's forward + backward of the PGX convolutional network on one MI355X: the training
kernels (`ConvNet.module(kernels=True)`) beside (a) the float64 twin `ConvNet.module()` on the same device and (b) the
same tower as plain torch `conv2d` under bf16 autocast, which is what a user would write instead.

    python tools/bench_pgx_conv_train.py [--reps 7] [--window-ms 30] [--out profiles/pgx_conv_train_bench.txt]

Per setting -- an Othello ConvNet (8 x 8 x 2, A = 65, P = 4, L = 4) at D = 64 with 4096 and 65536 rows and at D = 128
with 4096 and 16384 rows -- one JSON line.
A step is `integers(x)` (the tower: its forward), a loss in torch on p -- log-softmax cross-entropy over the A policy
columns plus the squared error of the value column -- and `backward()` down to every layer's weight and bias gradient;
no optimizer.  `*_us` is the device time between two events around `*_steps` back-to-back steps on torch's stream,
divided by that count: the median of `reps` windows taken in turns (kernels, twin, conv2d, kernels, ..) after a warm-up of
each, with the spread (max - min) / median.  Every form gets as many steps per window as make it `--window-ms` long by
a pilot step, and at least 3 (1 where a step takes over 0.1 s; a form whose step takes over 1 s gets two windows).  `gmacs` counts the multiply-accumulates of the three GEMMs per layer (forward, dx,
dW; no dx for the stem), from the shapes."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, C, A, P, L = 8, 8, 2, 65, 4, 4
SETTINGS = [(64, (4096, 65536)), (128, (4096, 16384))]  # D, rows


def macs_per_row(d):
    s = H * W
    return s * (2 * 9 * C * d + 3 * (2 * L * 9 * d * d + P * d)) + 3 * (A + 1) * s * P


def tower(torch, d, dev):
    conv = lambda k, n, size: torch.nn.Conv2d(k, n, size, padding=size // 2)

    class Tower(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.stem = conv(C, d, 3)
            self.blocks = torch.nn.ModuleList(
                [torch.nn.ModuleList([conv(d, d, 3), conv(d, d, 3)]) for _ in range(L)])
            self.reduce = conv(d, P, 1)
            self.head = torch.nn.Linear(H * W * P, A + 1)

        def forward(self, x):
            h = torch.relu(self.stem(x))
            for one, two in self.blocks:
                h = torch.relu(two(torch.relu(one(h))) + h)
            return self.head(torch.relu(self.reduce(h)).flatten(1))

    return Tower().to(dev).to(memory_format=torch.channels_last)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    from envpool_amd.pgx.net import ConvNet

    if not torch.cuda.is_available():
        raise SystemExit("bench_pgx_conv_train: needs a GPU")
    dev = torch.device("cuda", 0)
    lines = []
    a = A
    for d, row_counts in SETTINGS:
        net = ConvNet.random((H, W, C), A, d, L, P, seed=1)
        for rows in row_counts:
            rng = np.random.default_rng(rows)
            x = torch.tensor((rng.random((rows, H, W, C)) < 0.25).astype(np.uint8), device=dev)
            target = torch.tensor(rng.integers(0, a, rows), device=dev)
            z = torch.tensor(rng.uniform(-1, 1, rows), device=dev)
            fast, twin, plain = net.module(kernels=True).to(dev), net.module().to(dev), tower(torch, d, dev)
            x_half = x.to(torch.float32).permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)

            def loss_of(p, scale_p, scale_v):
                logp = torch.log_softmax(p[:, :a] * scale_p, dim=1)
                return -logp.gather(1, target[:, None]).mean() + ((p[:, a] * scale_v - z) ** 2).mean()

            def step_net(m):
                m.zero_grad(set_to_none=True)
                loss_of(m.integers(x), net.scale_p, net.scale_v).backward()

            def step_tower():
                plain.zero_grad(set_to_none=True)
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    p = plain(x_half)
                loss_of(p.float(), 1.0, 1.0).backward()

            forms = {"kernels": lambda: step_net(fast), "twin_f64": lambda: step_net(twin), "conv2d_bf16": step_tower}

            def window(step, steps):
                begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                begin.record()
                for _ in range(steps):
                    step()
                end.record()
                end.synchronize()
                return begin.elapsed_time(end) * 1e3 / steps

            for step in forms.values():  # warm-up: code objects, the handle, library algorithms
                step()
            torch.cuda.synchronize()
            # the two net paths agree before they are timed
            got, want = [w.grad.clone() for w in fast.weights], [w.grad for w in twin.weights]
            worst = max(float(((g - w).abs().max() / w.abs().max()).cpu()) for g, w in zip(got, want))
            pilot = {name: window(step, 1) for name, step in forms.items()}
            steps = {name: max(1 if pilot[name] > 1e5 else 3, math.ceil(args.window_ms * 1e3 / pilot[name]))
                     for name in forms}
            times = {name: [] for name in forms}
            for rep in range(args.reps):
                for name, step in forms.items():
                    if rep < 2 or pilot[name] < 1e6:  # (a form whose step takes seconds gets two windows)
                        times[name].append(window(step, steps[name]))
                print(f"rows {rows} D {d}: window {rep + 1} of {args.reps}", file=sys.stderr, flush=True)
            line = {"board": [H, W, C], "A": A, "D": d, "L": L, "P": P, "rows": rows, "window_ms": args.window_ms,
                    "gmacs": round(rows * macs_per_row(d) / 1e9, 2),
                    "worst_grad_diff_over_max": float(f"{worst:.3g}")}
            for name, ts in times.items():
                med = statistics.median(ts)
                line[name + "_us"] = round(med, 1)
                line[name + "_steps"] = steps[name]
                line[name + "_spread"] = round((max(ts) - min(ts)) / med, 3)
            line["twin_over_kernels"] = round(line["twin_f64_us"] / line["kernels_us"], 2)
            line["conv2d_over_kernels"] = round(line["conv2d_bf16_us"] / line["kernels_us"], 2)
            print(json.dumps(line), flush=True)
            lines.append(json.dumps(line))
            del fast, twin, plain
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# tools/bench_pgx_conv_train.py on one MI355X: device time of forward + loss + backward of one step, "
                     "the training kernels beside the float64 twin and the same tower as bf16-autocast torch conv2d\n")
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
