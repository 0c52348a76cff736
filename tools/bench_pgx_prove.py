"""The proven values of the PGX guided search (`prove=True`) on one MI355X: what an advance costs with the climb and
the closed picks in it, which share of the roots is proven by the end of the round, and the descents and model rows
that rules 4 and 5 save.

    python tools/bench_pgx_prove.py [--games ConnectFour,Othello] [--sizes 4096] [--widths 1,8] [--depths 0,1,2]
                                    [--tactics-nodes 4096] [--reps 3] [--warmup 1] [--out FILE]

The positions, S = 64, the device-side stand-in evaluator and the timing are those of tools/bench_pgx_tactics.py
(ConnectFour 10, Othello 44 seeded random legal plies from the reset); per game, k, width W and horizon D one JSON line
with both sessions, `prove` off and on:
  counting   a first session of each kind reads the statuses after every launch: the advances until the round is
             complete, the model rows (leaves of status 0 handed out, the k roots of advance 0 aside), and at the end
             the descents (the root visits summed: completed simulations) and, with `prove`, the roots whose proof is set
  advance    `reps` sessions after `warmup`, every advance between its own pair of events on the pool's stream (the
             evaluator outside the pair; with D > 0 PgxGuidedTactics inside it); the median over all of them and the
             spread of the per-session medians
  saved      descents and model rows of the session without `prove` minus those with it
The pick reads the children's two words (State.done, term0); the edge-flag form was not built, so there is no second
time to put beside this one."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_pgx_tactics import C_PUCT, S, rolled_pool  # noqa: E402


def measure(torch, pool, k, width, depth, prove, args):
    dev = torch.device("cuda", pool.device)
    stream = torch.cuda.ExternalStream(pool.stream, device=dev)
    h, w, c, a = pool.guided_shape()
    rows = k * width
    obs = torch.empty((rows, h, w, c), dtype=torch.bool, device=dev)
    mask = torch.empty((rows, a), dtype=torch.bool, device=dev)
    status = torch.empty((rows,), dtype=torch.uint8, device=dev)
    visits = torch.empty((k, a), dtype=torch.int32, device=dev)
    vals = torch.empty((k, a), dtype=torch.float32, device=dev)
    action = torch.empty((k,), dtype=torch.int32, device=dev)
    gen = torch.Generator().manual_seed(7)
    w_p = torch.randn((h * w * c, a), generator=gen).to(dev)
    w_v = (torch.randn((h * w * c,), generator=gen) * 0.2).to(dev)
    torch.cuda.synchronize(dev)

    def evaluate():
        x = obs.reshape(rows, -1).to(torch.float32)
        e = torch.exp(8.0 * torch.cos(x @ w_p)) * mask.to(torch.float32)
        return (e / e.sum(1, keepdim=True).clamp_min(1e-30)).contiguous(), torch.tanh(x @ w_v).contiguous()

    def begin():
        pool.guided_begin_device(obs.data_ptr(), mask.data_ptr(), status.data_ptr(), None, S, C_PUCT, 0,
                                 width if width > 1 else None, depth, args.tactics_nodes, prove)

    def advance(priors, values):
        pool.guided_advance_device(priors.data_ptr(), values.data_ptr(), rows, obs.data_ptr(), mask.data_ptr(),
                                   status.data_ptr())

    def event():
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(stream)
        return ev

    with torch.cuda.stream(stream):
        begin()
        advances, evaluated = 0, 0
        while bool((status != 2).any()):
            if advances > 0:
                evaluated += int((status == 0).sum())
            advance(*evaluate())
            advances += 1
            assert advances <= S + 1
        pool.guided_result_device(visits.data_ptr(), vals.data_ptr(), action.data_ptr())
        torch.cuda.synchronize(dev)
        descents = int(visits.sum())
        proven = int((pool.guided_proof()[0] != -128).sum())
        launches, medians = [], []
        for rep in range(args.warmup + args.reps):
            timed = []
            begin()
            for t in range(advances):
                priors, values = evaluate()
                e0 = event()
                advance(priors, values)
                timed.append((e0, event()))
            torch.cuda.synchronize(dev)
            assert bool((status == 2).all())
            if rep >= args.warmup:
                ms = [x.elapsed_time(y) for x, y in timed]
                launches += ms
                medians.append(float(np.median(ms)))
        pool.guided_end()
    return {"advances": advances, "advance_us_per_launch": round(float(np.median(launches)) * 1e3, 2),
            "advance_us_session_medians": [round(x * 1e3, 2) for x in medians], "model_rows": evaluated,
            "descents": descents, "proven_roots": proven}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", default="ConnectFour,Othello")
    ap.add_argument("--sizes", default="4096")
    ap.add_argument("--widths", default="1,8")
    ap.add_argument("--depths", default="0,1,2")
    ap.add_argument("--tactics-nodes", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from envpool_amd.core.device_pool import DevicePool

    if not torch.cuda.is_available():
        raise SystemExit("bench_pgx_prove: no GPU")
    out = open(args.out, "w") if args.out else None
    for fam in args.games.split(","):
        for k in [int(x) for x in args.sizes.split(",")]:
            pool = rolled_pool(DevicePool, fam, k)
            for width in [int(x) for x in args.widths.split(",")]:
                for depth in [int(x) for x in args.depths.split(",")]:
                    off = measure(torch, pool, k, width, depth, False, args)
                    on = measure(torch, pool, k, width, depth, True, args)
                    line = json.dumps({"game": fam, "roots": k, "simulations": S, "width": width, "tactics": depth,
                                       "off": off, "on": on,
                                       "proven_share": round(on["proven_roots"] / k, 4),
                                       "descents_saved": off["descents"] - on["descents"],
                                       "model_rows_saved": off["model_rows"] - on["model_rows"]})
                    print(line, flush=True)
                    if out:
                        out.write(line + "\n")
                        out.flush()
            pool.close()


if __name__ == "__main__":
    main()
