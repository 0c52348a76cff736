"""The PGX self-play recorder on one MI355X: the time of one `add` and of one `finish` in the device forms, beside one
`advance` launch of a guided search of the same pool, so that the price of the training samples can be read as a share
of the search that produces them.

    python tools/bench_pgx_record.py [--games Othello,Hex] [--k 4096] [--reps 5] [--symmetries 0,1] [--out FILE]

Per game, k envs and symmetries flag, one JSON line.  Every timed call sits between its own pair of events on the
pool's stream; the inputs are tensors made once, so nothing else runs between the events.  In front of the first event
the stream is given `--sleep-cycles` of idle spinning (default 400000, some 0.2 ms; 0: none), so that the host has
enqueued the call before the device reaches it: the figures are device times, not the host's launch path -- for the
advance launch and the recorder's calls alike.
  advance   a PUCT session of S = 64 on the freshly reset pool, constant priors: the median of its S + 1
            `guided_advance_device` launches (what tools/bench_guided.py reports), measured first in the same run
  staging   per rep the pool is reset, the recorder's staging discarded, and `plies` plies are staged: `add` of a fixed
            random policy tensor, then one committed playout ply (`playout_device(max_plies=1, commit=True)`) to move
            every env on.  `plies` is chosen per game so that no game can have ended (TicTacToe 4, ConnectFour 6) or few
            have (Hex 60, Othello 40); the staged plies are read from the counters afterwards.
  add       the median over all `DevicePool.record_add_device` calls of the reps (the pool's own call, as for the
            advance: the stream ordering of the torch wrappers is not between the events); bytes = k x (State 64 +
            policy 4 A) read and k x (State 64 + elapsed 4 + padded policy row) written
  finish    `DevicePool.record_finish_device` with `done` set for 0 %, 5 % (every 20th row) and 100 % of the rows, once per
            rep on freshly staged envs (the 0 % call changes nothing and is timed `reps` times on one staging); the
            median, the samples written per call and bytes = the staged rows read + the samples' seven arrays written
  typical   add + the 5 % finish, and that sum over the advance launch
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, C_PUCT = 64, 1.25
PLIES = {"TicTacToe": 4, "ConnectFour": 6, "Hex": 60, "Othello": 40}
NSYM = {"TicTacToe": 8, "ConnectFour": 2, "Hex": 2, "Othello": 8}


def median(xs):
    return float(np.median(xs)) if len(xs) else float("nan")


def measure(torch, ti, DevicePool, fam, k, sym, args):
    pool = DevicePool(fam, k, seed=0)
    dev = torch.device("cuda", pool.device)
    stream = torch.cuda.ExternalStream(pool.stream, device=dev)
    ids = torch.arange(k, dtype=torch.int32, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if args.sleep_cycles > 0:  # the stream is kept busy while the host prepares the call (see above)
            with torch.cuda.stream(stream):
                torch.cuda._sleep(args.sleep_cycles)
        e0.record(stream)
        fn()
        e1.record(stream)
        return e0, e1

    def reset():
        ti.send_device_tensors(pool, None, ids)
        ti.recv_device_tensors(pool)

    reset()
    h, w, c, a = pool.guided_shape()
    # -- the yardstick: one advance launch of a guided search of this pool
    obs = torch.empty((k, h, w, c), dtype=torch.bool, device=dev)
    mask = torch.empty((k, a), dtype=torch.bool, device=dev)
    status = torch.empty((k,), dtype=torch.uint8, device=dev)
    priors = torch.full((k, a), 1.0 / a, dtype=torch.float32, device=dev)
    values = torch.zeros((k,), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    advance = []
    for rep in range(1 + args.reps):
        pool.guided_begin_device(obs.data_ptr(), mask.data_ptr(), status.data_ptr(), None, S, C_PUCT)
        evs = [timed(lambda: pool.guided_advance_device(priors.data_ptr(), values.data_ptr(), k, obs.data_ptr(),
                                                        mask.data_ptr(), status.data_ptr())) for _ in range(S + 1)]
        torch.cuda.synchronize(dev)
        if rep >= 1:
            advance += [e0.elapsed_time(e1) for e0, e1 in evs]
    pool.guided_end()
    # -- the recorder
    plies = PLIES[fam]
    nsym = NSYM[fam] if sym else 1
    assert pool.record_begin(k * plies * nsym, max_plies=0, symmetries=bool(sym))[4] == nsym
    policy = torch.rand((k, a), dtype=torch.float32, device=dev)
    reward = torch.tensor([1.0, -1.0], dtype=torch.float32, device=dev).repeat(k, 1).contiguous()
    dones = {}
    for pct in (0, 5, 100):
        d = torch.zeros((k,), dtype=torch.bool, device=dev)
        if pct == 5:
            d[::20] = True
        elif pct == 100:
            d[:] = True
        dones[pct] = d
    torch.cuda.synchronize(dev)
    adds, finishes, samples, staged = [], {0: [], 5: [], 100: []}, {}, 0
    seed = 0
    for rep in range(1 + args.reps):
        for pct in (5, 100, 0):
            reset()
            pool.record_discard(None)
            ti.recorder_clear(pool)
            before = pool.record_counters()
            evs = []
            for t in range(plies):
                evs.append(timed(lambda: pool.record_add_device(policy.data_ptr())))
                seed += 1
                ti.playout_device(pool, None, 1, 1, seed, commit=True)
            n_fin = args.reps if pct == 0 else 1
            fin = [timed(lambda: pool.record_finish_device(reward.data_ptr(), dones[pct].data_ptr()))
                   for _ in range(n_fin)]
            torch.cuda.synchronize(dev)
            after = pool.record_counters()
            if rep >= 1:
                adds += [e0.elapsed_time(e1) for e0, e1 in evs]
                finishes[pct] += [e0.elapsed_time(e1) for e0, e1 in fin]
                samples[pct] = int(after[1] - before[1])
                assert int(after[3] - before[3]) == 0, "the capacity was sized for every staged ply"
                if pct == 100:
                    staged = samples[pct] // nsym
    pool.record_end()
    pool.close()
    ps = (a + 3) // 4 * 4
    add_bytes = k * (64 + 4 * a) + k * (64 + 4 + 4 * ps)
    row_bytes = h * w * c + a + 4 * a + 13

    def finish_bytes(n):
        return n // nsym * (64 + 4 + 4 * ps) + n * row_bytes + k * 17

    add_us, adv_us = 1e3 * median(adds), 1e3 * median(advance)
    out = dict(game=fam, k=k, symmetries=nsym, plies_per_env=plies, staged_plies=staged,
               advance_us_per_launch=round(adv_us, 2), add_us_per_call=round(add_us, 2), add_bytes=add_bytes,
               add_gb_per_s=round(add_bytes / add_us / 1e3, 1))
    for pct in (0, 5, 100):
        us = 1e3 * median(finishes[pct])
        out[f"finish_{pct}_us_per_call"] = round(us, 2)
        out[f"finish_{pct}_samples"] = samples[pct]
        out[f"finish_{pct}_bytes"] = finish_bytes(samples[pct])
        out[f"finish_{pct}_gb_per_s"] = round(finish_bytes(samples[pct]) / us / 1e3, 1)
    typical = add_us + out["finish_5_us_per_call"]
    out["typical_us_per_ply"] = round(typical, 2)
    out["typical_over_advance"] = round(typical / adv_us, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", default="TicTacToe,ConnectFour,Hex,Othello")
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--symmetries", default="0,1")
    ap.add_argument("--sleep-cycles", type=int, default=400000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from envpool_amd import torch_interop as ti
    from envpool_amd.core.device_pool import DevicePool

    if not torch.cuda.is_available():
        raise SystemExit("bench_pgx_record: no GPU (there is no CPU fallback)")
    lines = []
    for fam in args.games.split(","):
        for sym in (int(s) for s in args.symmetries.split(",")):
            lines.append(json.dumps(measure(torch, ti, DevicePool, fam, args.k, sym, args)))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
