"""Device time of forward + backward of a memory actor's `unroll` on one MI355X: the training kernels
(`unroll(..., kernels=True)`) beside the float64 twin (`unroll(...)`) on the same device.

    python tools/bench_actor_memory_train.py [--envs 4096,32768] [--horizon 32] [--reps 5] [--window-ms 30]
                                             [--out profiles/actor_memory_train_bench.txt]

The actor is `Actor.random` for MiniGrid-DoorKey-16x16-v0 with memory 64 and hidden 64; the observations are random
within the features' range (the time does not depend on them), the masks end 2 % of the slots.  A step is `unroll`, a
loss in torch -- the log-probability of random actions plus the squared error of the value -- and `backward()` down to
every gradient of the cell, the trunk and h0; no optimizer.  `*_us` is the device time between two events around
`*_steps` back-to-back steps on torch's stream, divided by that count: the median of `reps` windows taken in turns
after a warm-up of each, with the spread (max - min) / median; every form gets as many steps per window as make it
`--window-ms` long by a pilot window, and at least 2."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TASK, MEMORY, HIDDEN = "MiniGrid-DoorKey-16x16-v0", 64, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="4096,32768")
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    import envpool_amd as envpool
    from envpool_amd.actor import Actor

    if not torch.cuda.is_available():
        raise SystemExit("bench_actor_memory_train: needs a GPU")
    dev = torch.device("cuda", 0)
    env = envpool.make(TASK, "gymnasium", num_envs=64)
    actor = Actor.random(env, hidden=HIDDEN, blocks=1, seed=1, memory=MEMORY)
    env.close()
    t, f, lines = args.horizon, actor.features, []
    for n in (int(v) for v in args.envs.split(",")):
        rng = np.random.default_rng(n)
        obs = torch.tensor(actor.lo + rng.integers(0, 128, (t, n, f)) / actor.scale, device=dev)
        h0 = torch.tensor(rng.integers(0, 128, (n, MEMORY)).astype(np.float64), device=dev, requires_grad=True)
        mask = torch.tensor(rng.random((t, n)) >= 0.02, device=dev)
        action = torch.tensor(rng.integers(0, actor.actions, t * n), device=dev)
        z = torch.tensor(rng.uniform(-1, 1, (t, n)), device=dev)
        m = actor.module().to(dev)

        def step(kernels):
            m.zero_grad(set_to_none=True)
            h0.grad = None
            logits, value, h = m.unroll(obs, h0, mask, kernels=kernels)
            loss = -m.logp_of(logits.reshape(t * n, -1), action).mean() + ((value - z) ** 2).mean() + h.mean()
            loss.backward()

        forms = {"kernels": lambda: step(True), "twin_f64": lambda: step(False)}

        def window(one, steps):
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            begin.record()
            for _ in range(steps):
                one()
            end.record()
            end.synchronize()
            return begin.elapsed_time(end) * 1e3 / steps

        grads = {}
        for name, one in forms.items():  # warm-up: code objects, the handles, library algorithms
            one(), one()
            grads[name] = [p.grad.clone() for p in (*m.cell_weights, *m.net.weights, h0)]
        torch.cuda.synchronize()
        worst = max(float(((g - w).abs().max() / w.abs().max()).cpu())
                    for g, w in zip(grads["kernels"], grads["twin_f64"]))
        steps = {name: max(2, math.ceil(args.window_ms * 1e3 / window(one, 2))) for name, one in forms.items()}
        times = {name: [] for name in forms}
        for _ in range(args.reps):
            for name, one in forms.items():
                times[name].append(window(one, steps[name]))
        line = {"task": TASK, "F": f, "M": MEMORY, "hidden": HIDDEN, "T": t, "N": n, "window_ms": args.window_ms,
                "worst_grad_diff_over_max": float(f"{worst:.3g}")}
        for name, ts in times.items():
            med = statistics.median(ts)
            line[name + "_us"] = round(med, 1)
            line[name + "_steps"] = steps[name]
            line[name + "_spread"] = round((max(ts) - min(ts)) / med, 3)
        line["twin_over_kernels"] = round(line["twin_f64_us"] / line["kernels_us"], 2)
        line["kernels_slot_rows_per_s"] = float(f"{t * n / (line['kernels_us'] * 1e-6):.3g}")
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# tools/bench_actor_memory_train.py on one MI355X: device time of forward + loss + backward of one "
                     "unroll of a memory actor, the training kernels beside the float64 twin on the same device\n")
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
