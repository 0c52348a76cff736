"""Tree search of the PGX games on one MI355X: the fused search kernel (device form) beside the same search driven from
Python through fork / send_device_tensors / playout_device, which is what a caller writes without it.

    python tools/bench_search.py [--games TicTacToe,ConnectFour,Hex,Othello] [--sizes 1024,16384] [--reps 7]
                                 [--warmup 2] [--loop-reps 3] [--out FILE]

Per game and k freshly reset roots, S = 64 simulations of R = 8 leaf playouts, one JSON line:
  search   `torch_interop.search_device`: after `warmup` launches, each of `reps` launches (a new seed for each) timed
           with its own pair of events on the pool's stream; the median, and simulations per second = k * S / median
  loop     the batched search a caller can build from public calls: a pool of k * (S + 1) envs in which env
           i * (S + 1) + n is node n of root i; the statistics, masks and movers of the nodes in torch tensors on the
           device; per simulation a descent in torch (one round of gathers, scores and an arg-max per tree level, the
           host looking once per level whether any root still descends), then for the roots that expand: `fork` of the
           parent's env into the new node's env, one `send_device_tensors` / `recv_device_tensors` step of the new
           envs, one `playout_device` of R repeats from them, and the backup in torch.  Host clock around whole
           searches ending in a device synchronise; the median of `loop-reps` searches after one that warms up.  (The
           loop seeds its playouts per simulation instead of taking repeats t * R ..: the same work, other draws.)
  idle leaf lanes   (64 - R) / 64: the share of a wave's lanes without a leaf playout of their own while the wave
           plays the leaf out
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, R, C_PUCT = 64, 8, 1.25


def kernel_times(torch, ti, DevicePool, fam, k, args):
    pool = DevicePool(fam, k, seed=0)
    dev = torch.device("cuda", pool.device)
    stream = torch.cuda.ExternalStream(pool.stream, device=dev)
    ids = torch.arange(k, dtype=torch.int32, device=dev)
    ti.send_device_tensors(pool, None, ids)  # reset: every env at the start of a game
    ti.recv_device_tensors(pool)
    for w in range(args.warmup):
        ti.search_device(pool, None, S, R, C_PUCT, 0, seed=1000 + w)
    torch.cuda.synchronize(dev)
    ms, visits = [], None
    for i in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        visits, _, _ = ti.search_device(pool, None, S, R, C_PUCT, 0, seed=i)
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    assert bool((visits.sum(1) == S).all())
    pool.close()
    return float(np.median(ms)), [round(x, 3) for x in ms]


def loop_search(torch, ti, pool, k, n_act, seed):
    """One batched search of k roots (the envs i * (S + 1), at the start of a game) from public calls."""
    dev = torch.device("cuda", pool.device)
    ar = torch.arange(k, device=dev)
    child = torch.full((k, S + 1, n_act), -1, dtype=torch.int64, device=dev)
    v = torch.zeros((k, S + 1, n_act), dtype=torch.float32, device=dev)
    w0 = torch.zeros((k, S + 1, n_act), dtype=torch.float32, device=dev)
    mask = torch.zeros((k, S + 1, n_act), dtype=torch.bool, device=dev)
    mover = torch.zeros((k, S + 1), dtype=torch.int64, device=dev)
    done = torch.zeros((k, S + 1), dtype=torch.bool, device=dev)
    term0 = torch.zeros((k, S + 1), dtype=torch.float32, device=dev)
    roots = (ar * (S + 1)).to(torch.int32)
    ti.send_device_tensors(pool, None, roots)
    out = ti.recv_device_tensors(pool)
    mask[:, 0] = out["info:legal_action_mask"].bool()
    mover[:, 0] = out["info:current_player"].long()
    neg = torch.tensor(float("-inf"), device=dev)
    for t in range(S):
        node = torch.zeros(k, dtype=torch.int64, device=dev)
        active = torch.ones(k, dtype=torch.bool, device=dev)
        val = torch.zeros(k, dtype=torch.float32, device=dev)
        parent = torch.full((k,), -1, dtype=torch.int64, device=dev)
        parent_act = torch.zeros(k, dtype=torch.int64, device=dev)
        path = []
        while True:
            over = done[ar, node]
            val = torch.where(active & over, R * term0[ar, node], val)
            active = active & ~over
            if not bool(active.any()):
                break
            vv, ww = v[ar, node], w0[ar, node]
            sign = torch.where(mover[ar, node] == 0, 1.0, -1.0).unsqueeze(1)
            q = torch.where(vv > 0, sign * ww / (vv * R).clamp(min=1.0), torch.zeros_like(vv))
            score = q + C_PUCT * vv.sum(1, keepdim=True).sqrt() / (1.0 + vv)
            act = torch.where(mask[ar, node], score, neg).argmax(1)
            path.append((node, act, active))
            nxt = child[ar, node, act]
            need = active & (nxt < 0)
            parent = torch.where(need, node, parent)
            parent_act = torch.where(need, act, parent_act)
            active = active & ~need
            node = torch.where(active, nxt, node)
        grow = torch.nonzero(parent >= 0).reshape(-1)
        if len(grow):
            src = (grow * (S + 1) + parent[grow]).to(torch.int32)
            dst = (grow * (S + 1) + (t + 1)).to(torch.int32)
            dst_host = dst.cpu().numpy()
            ti.fork(pool, src.cpu().numpy(), dst_host, rng=False)
            ti.send_device_tensors(pool, parent_act[grow].to(torch.int32), dst)
            out = ti.recv_device_tensors(pool)
            rw0 = out["reward"].reshape(len(grow), 2)[:, 0].float()
            new_done = out["done"].bool().reshape(-1)
            child[grow, parent[grow], parent_act[grow]] = t + 1
            mask[grow, t + 1] = out["info:legal_action_mask"].bool()
            mover[grow, t + 1] = out["info:current_player"].long().reshape(-1)
            done[grow, t + 1] = new_done
            term0[grow, t + 1] = rw0
            ret, _, _ = ti.playout_device(pool, dst_host, repeats=R, seed=seed * S + t)
            val[grow] = torch.where(new_done, R * rw0, ret[:, :, 0].sum(1))
        for nodes, acts, took in path:
            f = took.float()
            v[ar, nodes, acts] += f
            w0[ar, nodes, acts] += f * val
    torch.cuda.synchronize(dev)
    assert bool((v[:, 0].sum(1) == S).all())


def loop_times(torch, ti, DevicePool, fam, k, n_act, args):
    pool = DevicePool(fam, k * (S + 1), seed=0)
    secs = []
    for rep in range(args.loop_reps + 1):  # the first one warms up
        torch.cuda.synchronize(torch.device("cuda", pool.device))
        t0 = time.perf_counter()
        loop_search(torch, ti, pool, k, n_act, rep)
        if rep > 0:
            secs.append(time.perf_counter() - t0)
    pool.close()
    return float(np.median(secs)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", default="TicTacToe,ConnectFour,Hex,Othello")
    ap.add_argument("--sizes", default="1024,16384")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from envpool_amd import torch_interop as ti
    from envpool_amd.core.device_pool import DevicePool

    sink = open(args.out, "w") if args.out else None
    actions = {"TicTacToe": 9, "ConnectFour": 7, "Hex": 122, "Othello": 65}
    for fam in args.games.split(","):
        for k in [int(x) for x in args.sizes.split(",")]:
            ms, all_ms = kernel_times(torch, ti, DevicePool, fam, k, args)
            rec = {"game": fam, "roots": k, "simulations": S, "leaf_playouts": R, "search_ms_per_launch": round(ms, 3),
                   "search_ms_all": all_ms, "search_simulations_per_s": float(k * S / (ms * 1e-3)),
                   "idle_leaf_lanes": (64 - R) / 64}
            if args.loop_reps > 0:
                loop_ms = loop_times(torch, ti, DevicePool, fam, k, actions[fam], args)
                rec.update({"loop_ms_per_search": round(loop_ms, 2),
                            "loop_simulations_per_s": float(k * S / (loop_ms * 1e-3)),
                            "search_over_loop": round(loop_ms / ms, 2)})
            text = json.dumps(rec)
            print(text, flush=True)
            if sink:
                sink.write(text + "\n")
                sink.flush()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
