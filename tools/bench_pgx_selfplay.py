"""Self-play of the PGX games on one MI355X: wall time per ply of the README's host-driven move loop against the
self-play driver (`env.selfplay(net).run`).

    python tools/bench_pgx_selfplay.py [--games Othello,Hex] [--k 4096] [--hidden 128] [--blocks 2] [--plies 60]
                                       [--warmup 5] [--reps 5] [--parent DIR] [--out profiles/pgx_selfplay_bench.txt]

Settings: Gumbel S = 32 plain and batch = 16, PUCT S = 64 width = 8; recorder open in both legs.
  a_host_ms_per_ply    the README's loop: `gumbel_search(seed=ply, ...).run(net)` (or `guided_search`), `rec.add`,
                       `env.step`, `rec.finish`, numpy in between.  With --parent DIR this leg imports the package from
                       DIR -- a checkout of the commit before the driver, built -- so that (a) is the parent's own.
  b_driver_ms_per_ply  `sp.run(plies, wait=False)` and a synchronise of the pool, on this tree
Each leg of each repeat is a process of its own (`--leg`), the legs alternate a, b, a, b, ...; the figure is the median
over the repeats of (wall time of `plies` plies, after `warmup` plies, ending in a synchronise) / plies, and `spread`
is (max - min) / median over the repeats of the same leg.  One JSON line per game and setting.

`--leg kernels` plays a few plies of every setting and nothing else: the program to put behind
`rocprofv3 --kernel-trace --stats --` for the device time of PgxSelfplayNoise / Move / Tally beside one advance.

    python tools/bench_pgx_selfplay.py --dirichlet 0.3 [--parent DIR] ...

measures what Dirichlet root noise costs a PUCT ply instead: leg `plain` is the PUCT setting of leg (b) without noise
(with --parent DIR on the parent's tree), leg `noisy` the same with `dirichlet_alpha` on this tree; same alternation,
median and spread.  The noise changes the games (without it all envs of a pool play one of two), so the difference is
the launch AND the other games; `--dirichlet-eps 0` runs the kernel and mixes nothing in, which leaves the launch.  `--leg noisy_kernels --dirichlet 0.3` is the program for rocprofv3 (PgxSelfplayDirichlet)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = [("gumbel", 32, {"max_considered": 16}), ("gumbel", 32, {"max_considered": 16, "batch": 16}),
            ("puct", 64, {"width": 8})]
SHAPE = {"TicTacToe": (3, 3, 2), "ConnectFour": (6, 7, 2), "Hex": (11, 11, 4), "Othello": (8, 8, 2)}
ACTIONS = {"TicTacToe": 9, "ConnectFour": 7, "Hex": 122, "Othello": 65}


def host_plies(np, env, rec, net, kind, s, kw, first, count):
    for ply in range(first, first + count):
        if kind == "gumbel":
            result = env.gumbel_search(simulations=s, seed=ply, **kw).run(net)
            target = result.weights
        else:
            result = env.guided_search(simulations=s, **kw).run(net)
            total = result.visits.sum(axis=1, keepdims=True)
            target = (result.visits / np.maximum(total, 1)).astype(np.float32)
        rec.add(target)
        _, rew, term, trunc, _ = env.step(np.where(result.action < 0, 0, result.action))
        rec.finish(rew, term | trunc)


def leg(args):
    """One leg in this process: a JSON line {setting key: ms per ply}."""
    sys.path.insert(0, args.root)
    import numpy as np

    import envpool_amd as envpool
    from envpool_amd.pgx.net import Net

    out = {}
    for fam in args.games.split(","):
        net = Net.random(SHAPE[fam], ACTIONS[fam], args.hidden, args.blocks, seed=0)
        for kind, s, kw in SETTINGS:
            if args.leg in ("plain", "noisy", "noisy_kernels"):
                if kind != "puct":
                    continue
                if args.leg != "plain":
                    kw = dict(kw, dirichlet_alpha=args.dirichlet, dirichlet_eps=args.dirichlet_eps)
            env = envpool.make(f"{fam}-v1", "gymnasium", num_envs=args.k, seed=7)
            rec = env.recorder(capacity=1 << 18)
            env.reset()
            key = f"{fam}/{kind}/S{s}/" + ",".join(f"{a}={b}" for a, b in kw.items())
            if args.leg == "host":
                host_plies(np, env, rec, net, kind, s, kw, 0, args.warmup)
                env.device_pool.synchronize()
                t0 = time.perf_counter()
                host_plies(np, env, rec, net, kind, s, kw, args.warmup, args.plies)
                env.device_pool.synchronize()
                out[key] = (time.perf_counter() - t0) * 1e3 / args.plies
            else:
                sp = env.selfplay(net, policy=kind, simulations=s, seed=0, **kw)
                sp.run(args.warmup)
                if args.leg in ("kernels", "noisy_kernels"):
                    sp.run(4)
                else:
                    t0 = time.perf_counter()
                    sp.run(args.plies, wait=False)
                    env.device_pool.synchronize()
                    out[key] = (time.perf_counter() - t0) * 1e3 / args.plies
                    out[key + "/games"] = sp.stats().games
                sp.close()
            rec.close()
            env.close()
    print("LEG " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", default="Othello,Hex")
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--plies", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit for leg (a)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, choices=["host", "driver", "kernels", "plain", "noisy", "noisy_kernels"])
    ap.add_argument("--dirichlet", type=float, default=0.0, help="alpha: measure the noise's cost per PUCT ply")
    ap.add_argument("--dirichlet-eps", type=float, default=0.25,
                    help="0: the kernel runs and mixes nothing in, so both legs play the same games")
    ap.add_argument("--root", default=HERE)
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    common = [sys.executable, os.path.abspath(__file__), "--games", args.games, "--k", str(args.k), "--hidden",
              str(args.hidden), "--blocks", str(args.blocks), "--plies", str(args.plies), "--warmup", str(args.warmup)]
    first, second = ("plain", "noisy") if args.dirichlet > 0 else ("host", "driver")
    common += ["--dirichlet", str(args.dirichlet), "--dirichlet-eps", str(args.dirichlet_eps)]
    runs = {first: [], second: []}
    for _ in range(args.reps):
        for name, root in ((first, args.parent or HERE), (second, HERE)):
            p = subprocess.run(common + ["--leg", name, "--root", os.path.abspath(root)], capture_output=True,
                               text=True, timeout=600, cwd=os.path.abspath(root))
            if p.returncode != 0:
                sys.exit(f"leg {name} failed ({p.returncode}):\n{p.stderr[-2000:]}")
            line = [x for x in p.stdout.splitlines() if x.startswith("LEG ")][-1]
            runs[name].append(json.loads(line[4:]))
    lines = []
    if args.dirichlet > 0:
        for key in [k for k in runs["plain"][0] if not k.endswith("/games")]:
            noisy = key + f",dirichlet_alpha={args.dirichlet},dirichlet_eps={args.dirichlet_eps}"
            rec = {"setting": noisy, "k": args.k, "hidden": args.hidden, "blocks": args.blocks, "plies": args.plies,
                   "reps": args.reps, "plain_tree": "parent" if args.parent else "this"}
            for name, col, kk in (("plain", "plain_ms_per_ply", key), ("noisy", "noisy_ms_per_ply", noisy)):
                xs = [r[kk] for r in runs[name]]
                med = statistics.median(xs)
                rec[col] = round(med, 4)
                rec[col.split("_ms")[0] + "_spread"] = round((max(xs) - min(xs)) / med, 3)
            rec["noisy_less_plain_us"] = round((rec["noisy_ms_per_ply"] - rec["plain_ms_per_ply"]) * 1e3, 1)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    for key in [] if args.dirichlet > 0 else [k for k in runs["driver"][0] if not k.endswith("/games")]:
        rec = {"setting": key, "k": args.k, "hidden": args.hidden, "blocks": args.blocks, "plies": args.plies,
               "reps": args.reps, "host_tree": "parent" if args.parent else "this"}
        for name, col in (("host", "a_host_ms_per_ply"), ("driver", "b_driver_ms_per_ply")):
            xs = [r[key] for r in runs[name]]
            med = statistics.median(xs)
            rec[col] = round(med, 3)
            rec[col.split("_ms")[0] + "_spread"] = round((max(xs) - min(xs)) / med, 3)
        rec["a_over_b"] = round(rec["a_host_ms_per_ply"] / rec["b_driver_ms_per_ply"], 2)
        rec["games_in_b"] = runs["driver"][0][key + "/games"]
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
