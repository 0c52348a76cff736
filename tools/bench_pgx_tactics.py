"""The exact leaf status of the PGX guided search (`tactics=D`) on one MI355X: what an advance costs with the solver's
launch behind it, which share of the handed-out leaves the solver decides, and how many positions it visits.

    python tools/bench_pgx_tactics.py [--games ConnectFour,Othello] [--sizes 4096] [--widths 1,8] [--depths 0,1,2,4]
                                      [--tactics-nodes 4096] [--reps 3] [--warmup 1] [--out FILE]

Per game, k roots (ConnectFour 10, Othello 44 seeded random legal plies from the reset; an env whose game ends on the
way starts a new one), width W, horizon D and S = 64 simulations in the device form, one JSON line.  The evaluator is
the device-side stand-in of tools/bench_guided.py (`hash`: peaked priors softmax(8 cos(obs . P)) over the legal actions
and values tanh(obs . v) from fixed random P, v) on the pool's stream.  D = 0 is a session without tactics: today's
launches.
  counting   a first session reads the statuses after every launch: the advances until the round is complete, the leaves
             of status 0 handed out for evaluation (the k roots of advance 0 aside), `decided` (search.decided summed)
             and the solver's visited positions (summed over the roots).  Positions and evaluator are fixed, so every
             later session makes exactly that many advances with no host wait.
  advance    after `warmup` whole sessions, `reps` sessions; every advance -- PgxGuidedAdvance(Wide) and, with D > 0,
             PgxGuidedTactics behind it -- sits between its own pair of events on the pool's stream (the evaluator is
             outside the pair); the median over all of them, min and max, and the spread of the per-session medians
  decided_share   decided / (decided + evaluated leaves): the share of the handed-out leaves that need no model
  solver_nodes_per_launch   the solver's visited positions per advance
The break-even against a model: the solver pays when  decided_share x (the model's time per row) x (rows per launch)
exceeds the added launch time  advance(D) - advance(0)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, C_PUCT = 64, 1.25
PLIES = {"ConnectFour": 10, "Othello": 44, "TicTacToe": 3, "Hex": 20}


def rolled_pool(DevicePool, fam, k):
    pool = DevicePool(fam, k, seed=0)
    ids = np.arange(k, dtype=np.int32)
    rng = np.random.default_rng(2)
    pool.reset(ids)
    mask = np.asarray(pool.recv_dict()["info:legal_action_mask"], bool)
    for _ in range(PLIES[fam]):
        pool.send(ids, (rng.random(mask.shape) * mask + mask).argmax(1).astype(np.int32))
        mask = np.asarray(pool.recv_dict()["info:legal_action_mask"], bool)
    return pool


def measure(torch, pool, fam, k, width, depth, args):
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
                                 width if width > 1 else None, depth, args.tactics_nodes)

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
        torch.cuda.synchronize(dev)
        decided, nodes = pool.guided_decided(with_nodes=True)
        decided, nodes = int(decided.sum()), int(nodes.sum())
        launches, medians = [], []
        for rep in range(args.warmup + args.reps):
            timed = []
            begin()
            for t in range(advances):
                priors, values = evaluate()
                e0 = event()
                advance(priors, values)
                timed.append((e0, event()))
            pool.guided_result_device(visits.data_ptr(), vals.data_ptr(), action.data_ptr())
            torch.cuda.synchronize(dev)
            assert bool((status == 2).all())
            if rep >= args.warmup:
                ms = [x.elapsed_time(y) for x, y in timed]
                launches += ms
                medians.append(float(np.median(ms)))
        pool.guided_end()
    return {"game": fam, "roots": k, "simulations": S, "width": width, "tactics": depth,
            "tactics_nodes": args.tactics_nodes if depth else 0, "advances": advances,
            "advance_us_per_launch": round(float(np.median(launches)) * 1e3, 2),
            "advance_us_min_max": [round(min(launches) * 1e3, 2), round(max(launches) * 1e3, 2)],
            "advance_us_session_medians": [round(x * 1e3, 2) for x in medians],
            "evaluated_leaves": evaluated, "decided": decided,
            "decided_share": round(decided / max(decided + evaluated, 1), 4),
            "solver_nodes": nodes, "solver_nodes_per_launch": round(nodes / max(advances, 1), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", default="ConnectFour,Othello")
    ap.add_argument("--sizes", default="4096")
    ap.add_argument("--widths", default="1,8")
    ap.add_argument("--depths", default="0,1,2,4")
    ap.add_argument("--tactics-nodes", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from envpool_amd.core.device_pool import DevicePool

    if not torch.cuda.is_available():
        raise SystemExit("bench_pgx_tactics: no GPU")
    out = open(args.out, "w") if args.out else None
    for fam in args.games.split(","):
        for k in [int(x) for x in args.sizes.split(",")]:
            pool = rolled_pool(DevicePool, fam, k)
            for width in [int(x) for x in args.widths.split(",")]:
                for depth in [int(x) for x in args.depths.split(",")]:
                    line = json.dumps(measure(torch, pool, fam, k, width, depth, args))
                    print(line, flush=True)
                    if out:
                        out.write(line + "\n")
                        out.flush()
            pool.close()


if __name__ == "__main__":
    main()
