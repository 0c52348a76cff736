"""Guided tree search of the PGX games on one MI355X: the time of one `advance` launch in the device form and the
roots x simulations per second of whole sessions, with a constant-prior evaluator so that the kernels are timed and
not a model; beside them `search()` with one leaf playout on the same positions.

    python tools/bench_guided.py [--games Othello,Hex] [--sizes 4096] [--reps 5] [--warmup 1] [--out FILE]

Per game and k freshly reset roots, S = 64 simulations, one JSON line:
  advance   after `warmup` whole sessions, `reps` sessions; every one of a session's S + 1 `guided_advance_device`
            launches sits between its own pair of events on the pool's stream; the median over all of them, and the
            median of the launches t = S/2 .. S-1 alone (deep trees).  The priors (1 / A everywhere) and values (0) are
            two tensors made once: no evaluator runs between the launches.
  session   one pair of events around a session's begin and all its advances; the median over the sessions, and
            roots x simulations per second = k * S / median
  search    `torch_interop.search_device(simulations=S, leaf_playouts=1)` on the same pool: 2 warm-up launches, then
            `reps` launches (a new seed each) each between its own pair of events; the median

    python tools/bench_guided.py --reroot [--games Othello,Hex] [--sizes 4096] [--reps 5] [--warmup 1] [--out FILE]

Tree reuse instead: per game and k freshly reset roots, S = 64 and nodes = 2 S + 1 = 129, one JSON line.  After `warmup`
whole sessions, `reps` sessions of 3 moves each: a full round of S + 1 advances, the result, and `guided_reroot_device`
by the most visited action (the result's action tensor, on the device), every launch between its own pair of events on
the pool's stream.
  reroot    the median over the reps x 3 reroot launches; beside it the median begin launch and the median advance
            launch of the same run
  kept      the share of a root's nodes that a reroot keeps, per move, averaged over the roots: (1 + the root's visits
            after the reroot) / (1 + its visits before) -- every simulation that did not end in a finished game made
            one node, so early in a game this is the node count itself

    python tools/bench_guided.py --width 1,4,8,16 [--evaluators const,hash] [--games Othello,Hex] [--sizes 64,4096] ...

Several leaves per launch instead: per game, k freshly reset roots, width W and evaluator, S = 64 in the device form, one
JSON line.  W = 1 is the plain session (S + 1 advances of k rows), the others are wide sessions (k W rows).
  evaluators  const: the two tensors above, nothing runs between the launches;  hash: a device-side evaluator on the
              pool's stream -- peaked priors softmax(8 cos(obs . P)) over the legal actions and values tanh(obs . v) from
              fixed random P, v -- so that descents collide as they do under a real policy
  advances    a first session reads the statuses after every launch and counts the advances until all of them are 2
              (and the leaves of status 0 handed out); the positions and the evaluator are fixed, so every later session
              makes exactly that many advances with no host wait
  advance     the median over all advance launches of `reps` sessions, each between its own pair of events (the
              evaluator is outside the pair); `vs_plain` = that median over W times the plain advance of the same game,
              k and evaluator (when W = 1 is in the same run): the cost of one wide launch in plain launches' worth of
              descents
  session     one pair of events around begin, all advances (and the evaluator's launches) and the result; the median

    python tools/bench_guided.py --gumbel --batch 1,4,16 [--simulations 32,64] [--considered 16] [--evaluators ..] ...

Gumbel sessions, a halving level per launch: per game, k freshly reset roots, S, batch B and evaluator, m = 16 in the
device form with fixed seeded noise, one JSON line.  B = 1 is the plain session (S + 1 advances of k rows), the others
are batch sessions (k B rows).  The evaluators are those of --width, as logits (const: zeros; hash: 8 cos(obs . P) on
the legal actions).  `advances`, `advance` and `session` as for --width; `vs_plain` = the median batch launch over B
times the plain Gumbel advance of the same game, k, S and evaluator; `puct_advance_us_per_launch` is the plain PUCT
advance (constant priors) of the same game, k and S, measured in the same run.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, C_PUCT = 64, 1.25


def measure(torch, ti, DevicePool, fam, k, args):
    pool = DevicePool(fam, k, seed=0)
    dev = torch.device("cuda", pool.device)
    stream = torch.cuda.ExternalStream(pool.stream, device=dev)
    ids = torch.arange(k, dtype=torch.int32, device=dev)
    ti.send_device_tensors(pool, None, ids)  # reset: every env at the start of a game
    ti.recv_device_tensors(pool)
    h, w, c, a = pool.guided_shape()
    obs = torch.empty((k, h, w, c), dtype=torch.bool, device=dev)
    mask = torch.empty((k, a), dtype=torch.bool, device=dev)
    status = torch.empty((k,), dtype=torch.uint8, device=dev)
    priors = torch.full((k, a), 1.0 / a, dtype=torch.float32, device=dev)
    values = torch.zeros((k,), dtype=torch.float32, device=dev)
    visits = torch.empty((k, a), dtype=torch.int32, device=dev)
    vals = torch.empty((k, a), dtype=torch.float32, device=dev)
    action = torch.empty((k,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    launches, deep, sessions = [], [], []
    for rep in range(args.warmup + args.reps):
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(S + 3)]
        evs[0].record(stream)
        pool.guided_begin_device(obs.data_ptr(), mask.data_ptr(), status.data_ptr(), None, S, C_PUCT)
        evs[1].record(stream)
        for t in range(S + 1):
            pool.guided_advance_device(priors.data_ptr(), values.data_ptr(), k, obs.data_ptr(), mask.data_ptr(),
                                       status.data_ptr())
            evs[t + 2].record(stream)
        pool.guided_result_device(visits.data_ptr(), vals.data_ptr(), action.data_ptr())
        evs[-1].synchronize()
        torch.cuda.synchronize(dev)
        if rep >= args.warmup:
            ms = [evs[t + 1].elapsed_time(evs[t + 2]) for t in range(S + 1)]
            launches += ms
            deep += ms[S // 2:S]
            sessions.append(evs[0].elapsed_time(evs[-1]))
    assert bool((visits.sum(1) == S).all()) and bool((status == 2).all())
    pool.guided_end()
    for wu in range(2):
        ti.search_device(pool, None, S, 1, C_PUCT, 0, seed=1000 + wu)
    torch.cuda.synchronize(dev)
    search = []
    for i in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        ti.search_device(pool, None, S, 1, C_PUCT, 0, seed=i)
        e1.record(stream)
        e1.synchronize()
        search.append(e0.elapsed_time(e1))
    pool.close()
    session_ms = float(np.median(sessions))
    return {"game": fam, "roots": k, "simulations": S,
            "advance_us_per_launch": round(float(np.median(launches)) * 1e3, 2),
            "advance_us_per_launch_deep": round(float(np.median(deep)) * 1e3, 2),
            "advance_us_min_max": [round(min(launches) * 1e3, 2), round(max(launches) * 1e3, 2)],
            "session_ms": round(session_ms, 3), "session_ms_all": [round(x, 3) for x in sessions],
            "roots_simulations_per_s": float(k * S / (session_ms * 1e-3)),
            "search_r1_ms": round(float(np.median(search)), 3),
            "search_r1_roots_simulations_per_s": float(k * S / (float(np.median(search)) * 1e-3))}


def measure_reroot(torch, ti, DevicePool, fam, k, args):
    moves, nodes = 3, 2 * S + 1
    pool = DevicePool(fam, k, seed=0)
    dev = torch.device("cuda", pool.device)
    stream = torch.cuda.ExternalStream(pool.stream, device=dev)
    ids = torch.arange(k, dtype=torch.int32, device=dev)
    ti.send_device_tensors(pool, None, ids)  # reset: every env at the start of a game
    ti.recv_device_tensors(pool)
    h, w, c, a = pool.guided_shape()
    obs = torch.empty((k, h, w, c), dtype=torch.bool, device=dev)
    mask = torch.empty((k, a), dtype=torch.bool, device=dev)
    status = torch.empty((k,), dtype=torch.uint8, device=dev)
    priors = torch.full((k, a), 1.0 / a, dtype=torch.float32, device=dev)
    values = torch.zeros((k,), dtype=torch.float32, device=dev)
    visits = torch.empty((k, a), dtype=torch.int32, device=dev)
    kept_visits = torch.empty((k, a), dtype=torch.int32, device=dev)
    vals = torch.empty((k, a), dtype=torch.float32, device=dev)
    action = torch.empty((k,), dtype=torch.int32, device=dev)
    scratch = torch.empty((k,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    begins, advances, reroots, kept = [], [], [], [[] for _ in range(moves)]

    def event():
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(stream)
        return ev

    for rep in range(args.warmup + args.reps):
        timed = {"begin": [], "advance": [], "reroot": []}
        shares = []
        e0 = event()
        pool.guided_begin_device(obs.data_ptr(), mask.data_ptr(), status.data_ptr(), None, S, C_PUCT, nodes)
        timed["begin"].append((e0, event()))
        for move in range(moves):
            for t in range(S + 1):
                e0 = event()
                pool.guided_advance_device(priors.data_ptr(), values.data_ptr(), k, obs.data_ptr(), mask.data_ptr(),
                                           status.data_ptr())
                timed["advance"].append((e0, event()))
            pool.guided_result_device(visits.data_ptr(), vals.data_ptr(), action.data_ptr())
            e0 = event()
            pool.guided_reroot_device(action.data_ptr(), k, S, obs.data_ptr(), mask.data_ptr(), status.data_ptr())
            timed["reroot"].append((e0, event()))
            pool.guided_result_device(kept_visits.data_ptr(), vals.data_ptr(), scratch.data_ptr())
            torch.cuda.synchronize(dev)
            assert bool((visits.sum(1) >= S).all()) and bool((status == 0).all())
            shares.append(float(((1 + kept_visits.sum(1)).double() / (1 + visits.sum(1)).double()).mean()))
        if rep >= args.warmup:
            begins += [x.elapsed_time(y) for x, y in timed["begin"]]
            advances += [x.elapsed_time(y) for x, y in timed["advance"]]
            reroots += [x.elapsed_time(y) for x, y in timed["reroot"]]
            for move in range(moves):
                kept[move].append(shares[move])
        pool.guided_end()
    pool.close()
    return {"game": fam, "roots": k, "simulations": S, "nodes": nodes, "moves": moves,
            "reroot_us_per_launch": round(float(np.median(reroots)) * 1e3, 2),
            "reroot_us_min_max": [round(min(reroots) * 1e3, 2), round(max(reroots) * 1e3, 2)],
            "begin_us_per_launch": round(float(np.median(begins)) * 1e3, 2),
            "advance_us_per_launch": round(float(np.median(advances)) * 1e3, 2),
            "nodes_kept_share_per_move": [round(float(np.mean(x)), 4) for x in kept]}


def measure_wide(torch, ti, DevicePool, fam, k, width, evaluator, args, plain_us):
    pool = DevicePool(fam, k, seed=0)
    dev = torch.device("cuda", pool.device)
    stream = torch.cuda.ExternalStream(pool.stream, device=dev)
    ids = torch.arange(k, dtype=torch.int32, device=dev)
    ti.send_device_tensors(pool, None, ids)  # reset: every env at the start of a game
    ti.recv_device_tensors(pool)
    h, w, c, a = pool.guided_shape()
    rows = k * width
    obs = torch.empty((rows, h, w, c), dtype=torch.bool, device=dev)
    mask = torch.empty((rows, a), dtype=torch.bool, device=dev)
    status = torch.empty((rows,), dtype=torch.uint8, device=dev)
    visits = torch.empty((k, a), dtype=torch.int32, device=dev)
    vals = torch.empty((k, a), dtype=torch.float32, device=dev)
    action = torch.empty((k,), dtype=torch.int32, device=dev)
    const = (torch.full((rows, a), 1.0 / a, dtype=torch.float32, device=dev),
             torch.zeros((rows,), dtype=torch.float32, device=dev))
    gen = torch.Generator().manual_seed(7)
    w_p = torch.randn((h * w * c, a), generator=gen).to(dev)
    w_v = (torch.randn((h * w * c,), generator=gen) * 0.2).to(dev)
    torch.cuda.synchronize(dev)

    def evaluate():
        if evaluator == "const":
            return const
        x = obs.reshape(rows, -1).to(torch.float32)
        e = torch.exp(8.0 * torch.cos(x @ w_p)) * mask.to(torch.float32)
        return (e / e.sum(1, keepdim=True).clamp_min(1e-30)).contiguous(), torch.tanh(x @ w_v).contiguous()

    def begin():
        if width == 1:
            pool.guided_begin_device(obs.data_ptr(), mask.data_ptr(), status.data_ptr(), None, S, C_PUCT)
        else:
            pool.guided_begin_device(obs.data_ptr(), mask.data_ptr(), status.data_ptr(), None, S, C_PUCT, 0, width)

    def event():
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(stream)
        return ev

    with torch.cuda.stream(stream):
        # the session that counts: a host wait after every launch
        begin()
        advances, leaves = 0, 0
        while bool((status != 2).any()):
            leaves += int((status == 0).sum())
            priors, values = evaluate()
            pool.guided_advance_device(priors.data_ptr(), values.data_ptr(), rows, obs.data_ptr(), mask.data_ptr(),
                                       status.data_ptr())
            advances += 1
            assert advances <= S + 1
        pool.guided_result_device(visits.data_ptr(), vals.data_ptr(), action.data_ptr())
        torch.cuda.synchronize(dev)
        assert bool((visits.sum(1) == S).all())
        launches, sessions = [], []
        for rep in range(args.warmup + args.reps):
            timed = []
            first = event()
            begin()
            for t in range(advances):
                priors, values = evaluate()
                e0 = event()
                pool.guided_advance_device(priors.data_ptr(), values.data_ptr(), rows, obs.data_ptr(), mask.data_ptr(),
                                           status.data_ptr())
                timed.append((e0, event()))
            pool.guided_result_device(visits.data_ptr(), vals.data_ptr(), action.data_ptr())
            last = event()
            last.synchronize()
            torch.cuda.synchronize(dev)
            assert bool((visits.sum(1) == S).all()) and bool((status == 2).all())
            if rep >= args.warmup:
                launches += [x.elapsed_time(y) for x, y in timed]
                sessions.append(first.elapsed_time(last))
    pool.guided_end()
    pool.close()
    us = float(np.median(launches)) * 1e3
    out = {"game": fam, "roots": k, "simulations": S, "width": width, "evaluator": evaluator,
           "advances_per_round": advances, "leaves_per_launch_per_root": round(leaves / (advances * k), 3),
           "advance_us_per_launch": round(us, 2),
           "advance_us_min_max": [round(min(launches) * 1e3, 2), round(max(launches) * 1e3, 2)],
           "session_ms": round(float(np.median(sessions)), 3), "session_ms_all": [round(x, 3) for x in sessions]}
    if width == 1:
        plain_us[(fam, k, evaluator)] = us
    elif (fam, k, evaluator) in plain_us:
        out["vs_plain"] = round(us / (width * plain_us[(fam, k, evaluator)]), 3)
    return out


def puct_advance_us(torch, pool, stream, dev, k, sims, args):
    """The median plain PUCT advance launch of `pool` over `reps` sessions of `sims` simulations, constant priors."""
    h, w, c, a = pool.guided_shape()
    obs = torch.empty((k, h, w, c), dtype=torch.bool, device=dev)
    mask = torch.empty((k, a), dtype=torch.bool, device=dev)
    status = torch.empty((k,), dtype=torch.uint8, device=dev)
    priors = torch.full((k, a), 1.0 / a, dtype=torch.float32, device=dev)
    values = torch.zeros((k,), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    launches = []
    for rep in range(args.warmup + args.reps):
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(sims + 2)]
        pool.guided_begin_device(obs.data_ptr(), mask.data_ptr(), status.data_ptr(), None, sims, C_PUCT)
        evs[0].record(stream)
        for t in range(sims + 1):
            pool.guided_advance_device(priors.data_ptr(), values.data_ptr(), k, obs.data_ptr(), mask.data_ptr(),
                                       status.data_ptr())
            evs[t + 1].record(stream)
        evs[-1].synchronize()
        torch.cuda.synchronize(dev)
        if rep >= args.warmup:
            launches += [evs[t].elapsed_time(evs[t + 1]) for t in range(sims + 1)]
    pool.guided_end()
    return float(np.median(launches)) * 1e3


def measure_gumbel(torch, ti, DevicePool, fam, k, sims, batch, evaluator, args, plain_us, puct_us):
    m = args.considered
    pool = DevicePool(fam, k, seed=0)
    dev = torch.device("cuda", pool.device)
    stream = torch.cuda.ExternalStream(pool.stream, device=dev)
    ids = torch.arange(k, dtype=torch.int32, device=dev)
    ti.send_device_tensors(pool, None, ids)  # reset: every env at the start of a game
    ti.recv_device_tensors(pool)
    h, w, c, a = pool.guided_shape()
    rows = k * batch
    obs = torch.empty((rows, h, w, c), dtype=torch.bool, device=dev)
    mask = torch.empty((rows, a), dtype=torch.bool, device=dev)
    status = torch.empty((rows,), dtype=torch.uint8, device=dev)
    visits = torch.empty((k, a), dtype=torch.int32, device=dev)
    vals = torch.empty((k, a), dtype=torch.float32, device=dev)
    action = torch.empty((k,), dtype=torch.int32, device=dev)
    weights = torch.empty((k, a), dtype=torch.float32, device=dev)
    const = (torch.zeros((rows, a), dtype=torch.float32, device=dev),
             torch.zeros((rows,), dtype=torch.float32, device=dev))
    gen = torch.Generator().manual_seed(7)
    w_p = torch.randn((h * w * c, a), generator=gen).to(dev)
    w_v = (torch.randn((h * w * c,), generator=gen) * 0.2).to(dev)
    u = torch.rand((k, a), generator=gen).clamp_(1e-20, 1.0 - 1e-7)
    noise = (-torch.log(-torch.log(u))).to(dev).contiguous()
    if (fam, k, sims) not in puct_us:
        puct_us[(fam, k, sims)] = puct_advance_us(torch, pool, stream, dev, k, sims, args)
    torch.cuda.synchronize(dev)

    def evaluate():
        if evaluator == "const":
            return const
        x = obs.reshape(rows, -1).to(torch.float32)
        return (8.0 * torch.cos(x @ w_p) * mask.to(torch.float32)).contiguous(), torch.tanh(x @ w_v).contiguous()

    def begin():
        pool.gumbel_begin_device(noise.data_ptr(), obs.data_ptr(), mask.data_ptr(), status.data_ptr(), None, sims, m,
                                 batch=None if batch == 1 else batch)

    def result():
        pool.gumbel_result_device(visits.data_ptr(), vals.data_ptr(), action.data_ptr(), weights.data_ptr())

    def event():
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(stream)
        return ev

    with torch.cuda.stream(stream):
        # the session that counts: a host wait after every launch
        begin()
        advances, leaves = 0, 0
        while bool((status != 2).any()):
            leaves += int((status == 0).sum())
            logits, values = evaluate()
            pool.gumbel_advance_device(logits.data_ptr(), values.data_ptr(), rows, obs.data_ptr(), mask.data_ptr(),
                                       status.data_ptr())
            advances += 1
            assert advances <= sims + 1
        result()
        torch.cuda.synchronize(dev)
        assert bool((visits.sum(1) == sims).all())
        launches, sessions = [], []
        for rep in range(args.warmup + args.reps):
            timed = []
            first = event()
            begin()
            for t in range(advances):
                logits, values = evaluate()
                e0 = event()
                pool.gumbel_advance_device(logits.data_ptr(), values.data_ptr(), rows, obs.data_ptr(),
                                           mask.data_ptr(), status.data_ptr())
                timed.append((e0, event()))
            result()
            last = event()
            last.synchronize()
            torch.cuda.synchronize(dev)
            assert bool((visits.sum(1) == sims).all()) and bool((status == 2).all())
            if rep >= args.warmup:
                launches += [x.elapsed_time(y) for x, y in timed]
                sessions.append(first.elapsed_time(last))
    pool.guided_end()
    pool.close()
    us = float(np.median(launches)) * 1e3
    out = {"game": fam, "roots": k, "policy": "gumbel", "simulations": sims, "considered": m, "batch": batch,
           "evaluator": evaluator, "advances_per_round": advances,
           "leaves_per_launch_per_root": round(leaves / (advances * k), 3), "advance_us_per_launch": round(us, 2),
           "advance_us_min_max": [round(min(launches) * 1e3, 2), round(max(launches) * 1e3, 2)],
           "session_ms": round(float(np.median(sessions)), 3), "session_ms_all": [round(x, 3) for x in sessions],
           "puct_advance_us_per_launch": round(puct_us[(fam, k, sims)], 2)}
    if batch == 1:
        plain_us[(fam, k, sims, evaluator)] = us
    elif (fam, k, sims, evaluator) in plain_us:
        out["vs_plain"] = round(us / (batch * plain_us[(fam, k, sims, evaluator)]), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", default="Othello,Hex")
    ap.add_argument("--sizes", default="4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reroot", action="store_true", help="time guided_reroot_device instead (tree reuse)")
    ap.add_argument("--width", default=None, help="several leaves per launch instead: the widths, e.g. 1,4,8,16")
    ap.add_argument("--evaluators", default="const,hash", help="with --width or --gumbel: const, hash or both")
    ap.add_argument("--gumbel", action="store_true", help="Gumbel sessions instead, a halving level per launch")
    ap.add_argument("--batch", default="1,4,16", help="with --gumbel: the batches; 1 is the plain session")
    ap.add_argument("--simulations", default="32,64", help="with --gumbel: the simulations per move")
    ap.add_argument("--considered", type=int, default=16, help="with --gumbel: m")
    args = ap.parse_args()
    import torch

    from envpool_amd import torch_interop as ti
    from envpool_amd.core.device_pool import DevicePool

    sink = open(args.out, "w") if args.out else None
    plain_us, puct_us = {}, {}
    for fam in args.games.split(","):
        for k in [int(x) for x in args.sizes.split(",")]:
            if args.gumbel:
                for sims in [int(x) for x in args.simulations.split(",")]:
                    for evaluator in args.evaluators.split(","):
                        for batch in [int(x) for x in args.batch.split(",")]:
                            text = json.dumps(measure_gumbel(torch, ti, DevicePool, fam, k, sims, batch, evaluator,
                                                             args, plain_us, puct_us))
                            print(text, flush=True)
                            if sink:
                                sink.write(text + "\n")
                                sink.flush()
                continue
            if args.width:
                for evaluator in args.evaluators.split(","):
                    for width in [int(x) for x in args.width.split(",")]:
                        text = json.dumps(measure_wide(torch, ti, DevicePool, fam, k, width, evaluator, args,
                                                       plain_us))
                        print(text, flush=True)
                        if sink:
                            sink.write(text + "\n")
                            sink.flush()
                continue
            text = json.dumps((measure_reroot if args.reroot else measure)(torch, ti, DevicePool, fam, k, args))
            print(text, flush=True)
            if sink:
                sink.write(text + "\n")
                sink.flush()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
