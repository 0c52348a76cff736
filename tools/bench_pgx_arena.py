"""A match of two nets on the PGX games on one MI355X: wall time per ply of the host-driven two-net loop against the
arena (`env.arena(net_a, net_b).run`).

    python tools/bench_pgx_arena.py [--games Othello,Hex] [--k 4096] [--hidden 128] [--blocks 2] [--plies 60]
                                    [--warmup 5] [--reps 5] [--parent DIR] [--out profiles/pgx_arena_bench.txt]

Settings: Gumbel S = 32 plain and batch = 16, PUCT S = 64 width = 8; two nets of D = `hidden`, L = `blocks`; no recorder.
  a_host_ms_per_ply   the host-driven loop: noise rows from the self-play restatement (tests/pgx_selfplay_util.py) as
                      `gumbel=`, a session whose evaluate calls both `net.bind(env)` callables on ALL rows and selects by
                      the side restated from `info["current_player"]`, the restated move, `env.step`.  With --parent DIR
                      this leg imports the package from DIR -- a built checkout of the commit before the arena.
  b_arena_ms_per_ply  `arena.run(plies, wait=False)` and a synchronise of the pool, on this tree
Each leg of each repeat is a process of its own (`--leg`), the legs alternate a, b, a, b, ...; the figure is the median
over the repeats of (wall time of `plies` plies, after `warmup` plies, ending in a synchronise) / plies, and `spread`
is (max - min) / median over the repeats of the same leg.  One JSON line per game and setting.

`--leg kernels` makes, for rows in 4096 and 65536, twenty single-net evaluations and twenty pair evaluations (plan
included) of the same random rows with an alternating side, and nothing else: the program to put behind
`rocprofv3 --kernel-trace --stats --` for the device time of PgxNetPlanCount + PgxNetPlanPlace + PgxNetEval<true>
beside PgxNetEval<false>."""
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


def host_plies(np, SU, env, nets, kind, s, kw, first, count, state):
    """`count` plies of the match from Python; `state` carries (info, elapsed) between calls."""
    ids = np.asarray(env.all_env_ids)
    n = len(ids)
    both = [net.bind(env, kind == "puct") for net in nets]
    for ply in range(first, first + count):
        side = ((np.asarray(state["info"]["current_player"]).reshape(-1) ^ ids) & 1).astype(bool)

        def evaluate(obs, mask, status):
            (pa, va), (pb, vb) = (ev(obs, mask, status) for ev in both)
            width = pa.shape[-1]
            rows = pa.reshape(-1, width).shape[0]
            sel = np.repeat(side, rows // n)
            return (np.where(sel[:, None], pb.reshape(-1, width), pa.reshape(-1, width)).reshape(pa.shape),
                    np.where(sel, vb.reshape(-1), va.reshape(-1)).reshape(va.shape))

        if kind == "gumbel":
            noise = SU.noise_rows(0, ids, ply, state["actions"])
            result = env.gumbel_search(simulations=s, gumbel=noise, **kw).run(evaluate)
            action, _ = SU.gumbel_move(result.action, result.weights)
        else:
            result = env.guided_search(simulations=s, **kw).run(evaluate)
            action, _ = SU.puct_move(result.visits, result.action, state["elapsed"], 0, SU.key(0, ids, ply))
        _, _, _, _, info = env.step(action)
        state["info"], state["elapsed"] = info, np.asarray(info["elapsed_step"]).reshape(-1)


def kernels_leg(args, np, envpool, Net):
    from envpool_amd.core.device_pool import DevicePool

    fam = args.games.split(",")[0]
    f, a = int(np.prod(SHAPE[fam])), ACTIONS[fam]
    nets = [Net.random(SHAPE[fam], a, args.hidden, args.blocks, seed=i) for i in (0, 1)]
    pool = DevicePool(fam, 4, seed=1)
    rng = np.random.default_rng(0)
    for rows in (4096, 65536):
        obs = (rng.random((rows, f)) < 0.25).astype(np.uint8)
        mask = np.ones((rows, a), np.uint8)
        status = np.zeros(rows, np.uint8)
        side = (np.arange(rows) & 1).astype(np.uint8)
        for _ in range(20):
            pool.net_eval(nets[0], obs, mask, status, False)
            pool.net_eval_pair(nets[0], nets[1], obs, mask, status, side, False)
    pool.close()


def leg(args):
    """One leg in this process: a JSON line {setting key: ms per ply}."""
    sys.path.insert(0, args.root)
    sys.path.insert(0, os.path.join(args.root, "tests"))
    import numpy as np

    import envpool_amd as envpool
    from envpool_amd.pgx.net import Net

    if args.leg == "kernels":
        return kernels_leg(args, np, envpool, Net)
    import pgx_selfplay_util as SU

    out = {}
    for fam in args.games.split(","):
        nets = [Net.random(SHAPE[fam], ACTIONS[fam], args.hidden, args.blocks, seed=i) for i in (0, 1)]
        for kind, s, kw in SETTINGS:
            env = envpool.make(f"{fam}-v1", "gymnasium", num_envs=args.k, seed=7)
            _, info = env.reset()
            key = f"{fam}/{kind}/S{s}/" + ",".join(f"{a}={b}" for a, b in kw.items())
            if args.leg == "host":
                state = {"info": info, "elapsed": np.asarray(info["elapsed_step"]).reshape(-1),
                         "actions": ACTIONS[fam]}
                host_plies(np, SU, env, nets, kind, s, kw, 0, args.warmup, state)
                env.device_pool.synchronize()
                t0 = time.perf_counter()
                host_plies(np, SU, env, nets, kind, s, kw, args.warmup, args.plies, state)
                env.device_pool.synchronize()
                out[key] = (time.perf_counter() - t0) * 1e3 / args.plies
            else:
                arena = env.arena(nets[0], nets[1], policy=kind, simulations=s, seed=0, **kw)
                arena.run(args.warmup)
                t0 = time.perf_counter()
                arena.run(args.plies, wait=False)
                env.device_pool.synchronize()
                out[key] = (time.perf_counter() - t0) * 1e3 / args.plies
                out[key + "/games"] = arena.stats().games
                arena.close()
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
    ap.add_argument("--leg", default=None, choices=["host", "arena", "kernels"])
    ap.add_argument("--root", default=HERE)
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    common = [sys.executable, os.path.abspath(__file__), "--games", args.games, "--k", str(args.k), "--hidden",
              str(args.hidden), "--blocks", str(args.blocks), "--plies", str(args.plies), "--warmup", str(args.warmup)]
    runs = {"host": [], "arena": []}
    for _ in range(args.reps):
        for name, root in (("host", args.parent or HERE), ("arena", HERE)):
            p = subprocess.run(common + ["--leg", name, "--root", os.path.abspath(root)], capture_output=True,
                               text=True, timeout=600, cwd=os.path.abspath(root))
            if p.returncode != 0:
                sys.exit(f"leg {name} failed ({p.returncode}):\n{p.stderr[-2000:]}")
            line = [x for x in p.stdout.splitlines() if x.startswith("LEG ")][-1]
            runs[name].append(json.loads(line[4:]))
    lines = []
    for key in [k for k in runs["arena"][0] if not k.endswith("/games")]:
        rec = {"setting": key, "k": args.k, "hidden": args.hidden, "blocks": args.blocks, "plies": args.plies,
               "reps": args.reps, "host_tree": "parent" if args.parent else "this"}
        for name, col in (("host", "a_host_ms_per_ply"), ("arena", "b_arena_ms_per_ply")):
            xs = [r[key] for r in runs[name]]
            med = statistics.median(xs)
            rec[col] = round(med, 3)
            rec[col.split("_ms")[0] + "_spread"] = round((max(xs) - min(xs)) / med, 3)
        rec["a_over_b"] = round(rec["a_host_ms_per_ply"] / rec["b_arena_ms_per_ply"], 2)
        rec["games_in_b"] = runs["arena"][0][key + "/games"]
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
