"""Device time of one evaluation launch of the PGX convolutional network (PgxConvEval) on one MI355X, beside the same
tower as `torch.nn.functional.conv2d` in bf16 on the same device.

    python tools/bench_pgx_conv.py [--rows 4096,65536] [--reps 7] [--launches 10] [--out profiles/pgx_conv_bench.txt]

Per setting -- Othello D = 64, L = 4, P = 8 and Hex D = 64, L = 4, P = 4 -- and row count one JSON line: `conv_us`,
the device time between two events of `launches` back-to-back epa_net_eval_device launches on the pool's stream,
divided by `launches`; `torch_bf16_us`, the same for the torch tower (stem, L residual blocks, 1x1 reduce, dense head,
channels-last bf16, no gradients) on torch's stream; both the median of `reps` windows taken in turns (conv, torch,
conv, ..) after a warm-up of each, with the spread (max - min) / median.  `gmacs` is the int8 multiply-accumulates the
contract needs per launch, computed from the shapes; `share_of_peak` is `gmacs` over `conv_us` against the part's dense
int8 peak of 2.5e15 MAC/s (5.0 POPS).  Every row is evaluated (status 0, boards of density 1/4)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = [("Othello", 64, 4, 8), ("Hex", 64, 4, 4)]  # game, D, L, P
PEAK_MACS = 2.5e15


def macs_per_row(h, w, c, a, d, blocks, p):
    s = h * w
    return s * 9 * c * d + 2 * blocks * s * 9 * d * d + s * d * p + (a + 1) * s * p


def tower(torch, c, a, d, blocks, p, s, dev):
    conv = lambda i, o, k: torch.nn.Conv2d(i, o, k, padding=k // 2)  # noqa: E731

    class Tower(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.stem = conv(c, d, 3)
            self.blocks = torch.nn.ModuleList([torch.nn.ModuleList([conv(d, d, 3), conv(d, d, 3)]) for _ in range(blocks)])
            self.reduce = conv(d, p, 1)
            self.head = torch.nn.Linear(s * p, a + 1)

        def forward(self, x):
            h = torch.relu(self.stem(x))
            for one, two in self.blocks:
                h = torch.relu(two(torch.relu(one(h))) + h)
            g = torch.relu(self.reduce(h))
            return self.head(g.permute(0, 2, 3, 1).reshape(g.shape[0], -1))

    torch.manual_seed(0)
    return Tower().to(dev).to(torch.bfloat16).to(memory_format=torch.channels_last).eval()


def window(torch, stream, fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(launches):
        fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="4096,65536")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from envpool_amd.core.device_pool import DevicePool
    from envpool_amd.pgx.net import ConvNet

    lines = []
    for fam, d, blocks, p in SETTINGS:
        pool = DevicePool(fam, 64, seed=1)
        dev = torch.device("cuda", pool.device)
        h, w, c, a = pool.guided_shape()
        net = ConvNet.random((h, w, c), a, d, blocks, p, seed=0)
        model = tower(torch, c, a, d, blocks, p, h * w, dev)
        ours, theirs = torch.cuda.ExternalStream(pool.stream, device=dev), torch.cuda.current_stream(dev)
        for rows in (int(x) for x in args.rows.split(",")):
            boards = (torch.rand((rows, h, w, c), device=dev) < 0.25).contiguous()
            x = boards.permute(0, 3, 1, 2).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
            mask = torch.ones((rows, a), dtype=torch.bool, device=dev)
            status = torch.zeros((rows,), dtype=torch.uint8, device=dev)
            policy = torch.empty((rows, a), dtype=torch.float32, device=dev)
            value = torch.empty((rows,), dtype=torch.float32, device=dev)
            torch.cuda.synchronize(dev)

            def conv_launch():
                pool.net_eval_device(net, rows, False, boards.data_ptr(), mask.data_ptr(), status.data_ptr(),
                                     policy.data_ptr(), value.data_ptr())

            def torch_launch():
                with torch.no_grad():
                    model(x)

            for fn, stream in ((conv_launch, ours), (torch_launch, theirs)):  # warm-up of every shape
                window(torch, stream, fn, 3)
            t_conv, t_torch = [], []
            for _ in range(args.reps):  # in turns, never overlapping: each window ends in a wait for its last event
                t_conv.append(window(torch, ours, conv_launch, args.launches))
                t_torch.append(window(torch, theirs, torch_launch, args.launches))
            mc, mt = statistics.median(t_conv), statistics.median(t_torch)
            gmacs = rows * macs_per_row(h, w, c, a, d, blocks, p) / 1e9
            rec = {"game": fam, "D": d, "L": blocks, "P": p, "rows": rows, "conv_us": round(mc, 1),
                   "conv_spread": round((max(t_conv) - min(t_conv)) / mc, 3), "torch_bf16_us": round(mt, 1),
                   "torch_spread": round((max(t_torch) - min(t_torch)) / mt, 3), "torch_over_conv": round(mt / mc, 2),
                   "gmacs": round(gmacs, 2), "int8_tmacs_per_s": round(gmacs / mc * 1e3, 1),
                   "share_of_peak": round(gmacs * 1e9 / (mc * 1e-6) / PEAK_MACS, 4)}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        net.close()
        pool.close()
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
