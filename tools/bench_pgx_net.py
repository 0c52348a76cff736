"""One search round of the PGX games with the built-in network on one MI355X: what the evaluator costs between two
advance launches, three ways.

    python tools/bench_pgx_net.py [--games Othello,Hex] [--k 4096] [--hidden 128] [--blocks 2] [--reps 5]
                                  [--warmup 2] [--out profiles/pgx_net_bench.txt]

Per game (positions: tools/bench_pgx_tactics.py's seeded random plies) and setting -- Gumbel S = 32 plain and
batch = 16, PUCT S = 64 plain and width = 8 -- one JSON line with the wall time of a whole round (begin .. result,
device idle before and after), the median of `reps` after `warmup`, the spread as (max - min) / median:
  a_torch_mlp_ms   the torch_interop device forms with a float torch.nn MLP of the same F / D / L / A (trunk, L
                   residual blocks, head).  This leg uses nothing of the built-in network, so the same file run on the
                   commit before it gives the baseline.
  b_net_callable_ms  the same forms with the Net as a plain callable (`net.bind(pool)`): one PgxNetEval per model call,
                   still through Python and the two event orderings per launch
  c_run_net_ms     the forms with the Net itself: the round enqueued from C++ (epa_net_run)
and, per game, the device time between events of one PgxNetEval at k and at 16 k rows beside one advance launch of the
plain and of the batch / wide session (`eval_us`, `advance_us`).  Legs b and c are left out where the package has no
`envpool_amd.pgx.net`."""
import argparse
import json
import os
import statistics
import sys
import time


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_pgx_tactics import rolled_pool  # noqa: E402

SETTINGS = [("gumbel", 32, {}), ("gumbel", 32, {"batch": 16}), ("puct", 64, {}), ("puct", 64, {"width": 8})]


def mlp(torch, f, d, blocks, a, dev):
    class Mlp(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.trunk = torch.nn.Linear(f, d)
            self.blocks = torch.nn.ModuleList(
                [torch.nn.ModuleList([torch.nn.Linear(d, d), torch.nn.Linear(d, d)]) for _ in range(blocks)])
            self.head = torch.nn.Linear(d, a + 1)

        def forward(self, obs):
            h = torch.relu(self.trunk(obs.reshape(obs.shape[0], -1).to(torch.float32)))
            for one, two in self.blocks:
                h = torch.relu(two(torch.relu(one(h))) + h)
            return self.head(h)

    torch.manual_seed(0)
    return Mlp().to(dev).eval()


def timed(torch, dev, fn, reps, warmup):
    out = []
    for i in range(warmup + reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    med = statistics.median(out)
    return round(med, 3), round((max(out) - min(out)) / med, 3)


def device_us(torch, pool, dev, fn, reps=20):
    stream = torch.cuda.ExternalStream(pool.stream, device=dev)
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return round(statistics.median(out), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", default="Othello,Hex")
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from envpool_amd import torch_interop as ti
    from envpool_amd.core.device_pool import DevicePool

    try:
        from envpool_amd.pgx.net import Net
    except ImportError:
        Net = None
    lines = []
    for fam in args.games.split(","):
        pool = rolled_pool(DevicePool, fam, args.k)
        dev = torch.device("cuda", pool.device)
        h, w, c, a = pool.guided_shape()
        f = h * w * c
        model = mlp(torch, f, args.hidden, args.blocks, a, dev)
        net = Net.random((h, w, c), a, args.hidden, args.blocks, seed=0) if Net is not None else None

        def torch_eval(priors):
            def evaluate(obs, mask, status):
                with torch.no_grad():
                    out = model(obs)
                logits, value = out[:, :a], torch.tanh(out[:, a])
                if priors:
                    logits = torch.softmax(logits.masked_fill(~mask, -1e30), dim=1) * mask
                return logits, value
            return evaluate

        for kind, s, kw in SETTINGS:
            noise = torch.zeros((args.k, a), dtype=torch.float32, device=dev)

            def round_(evaluate):
                if kind == "gumbel":
                    return ti.gumbel_search_device(pool, evaluate, None, s, 16, gumbel=noise, **kw)
                return ti.guided_search_device(pool, evaluate, None, s, **kw)

            rec = {"game": fam, "k": args.k, "policy": kind, "simulations": s, **kw, "hidden": args.hidden,
                   "blocks": args.blocks}
            rec["a_torch_mlp_ms"], rec["a_spread"] = timed(torch, dev, lambda: round_(torch_eval(kind == "puct")),
                                                          args.reps, args.warmup)
            if net is not None:
                bound = net.bind(pool, priors=kind == "puct")
                rec["b_net_callable_ms"], rec["b_spread"] = timed(torch, dev, lambda: round_(bound), args.reps,
                                                                  args.warmup)
                rec["c_run_net_ms"], rec["c_spread"] = timed(torch, dev, lambda: round_(net), args.reps, args.warmup)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        if net is not None:
            rec = {"game": fam, "k": args.k, "hidden": args.hidden, "blocks": args.blocks}
            for mult in (1, 16):
                rows = args.k * mult
                obs = torch.zeros((rows, h, w, c), dtype=torch.bool, device=dev)
                mask = torch.ones((rows, a), dtype=torch.bool, device=dev)
                status = torch.zeros((rows,), dtype=torch.uint8, device=dev)
                noise = torch.zeros((args.k, a), dtype=torch.float32, device=dev)
                pool.gumbel_begin_device(noise.data_ptr(), obs.data_ptr(), mask.data_ptr(), status.data_ptr(), None, 32,
                                         16, batch=16 if mult > 1 else None)
                policy = torch.empty((rows, a), dtype=torch.float32, device=dev)
                value = torch.empty((rows,), dtype=torch.float32, device=dev)
                torch.cuda.synchronize(dev)
                # (every row evaluated: random boards of density 1/4 and statuses 0, not the session's leaves)
                boards = (torch.rand((rows, h, w, c), device=dev) < 0.25).contiguous()
                zeros = torch.zeros((rows,), dtype=torch.uint8, device=dev)
                torch.cuda.synchronize(dev)
                rec[f"eval_us_rows_{rows}"] = device_us(torch, pool, dev, lambda: pool.net_eval_device(
                    net, rows, False, boards.data_ptr(), mask.data_ptr(), zeros.data_ptr(), policy.data_ptr(),
                    value.data_ptr()))
                pool.net_eval_device(net, rows, False, obs.data_ptr(), mask.data_ptr(), status.data_ptr(),
                                     policy.data_ptr(), value.data_ptr())
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                stream = torch.cuda.ExternalStream(pool.stream, device=dev)
                e0.record(stream)
                pool.gumbel_advance_device(policy.data_ptr(), value.data_ptr(), rows, obs.data_ptr(), mask.data_ptr(),
                                           status.data_ptr())
                e1.record(stream)
                e1.synchronize()
                rec[f"advance_us_rows_{rows}"] = round(e0.elapsed_time(e1) * 1e3, 2)
                pool.guided_end()
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        pool.close()
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
