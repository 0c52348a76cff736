"""`ro.collect()` against the same horizon driven from Python, on the device path.

For CartPole-v1 and HalfCheetah-v4 at num_envs = 65536 and a horizon of T = 32 it times one horizon
  collect   rollout_collect_device (features, the int8 net, the sample, the step and the collector's kernels per step,
            all enqueued from C++), rollout_gae with the stored values, rollout_next
  loop      the way without the actor: T x (`actor.module()` on the device as the policy -- features, the integer net in
            float64, sampling and log-probability in torch --, rollout_step_device), rollout_gae_device on the values
            kept in a torch tensor, rollout_next
and prints one JSON line per env: env-steps/s of both (median of `--repeats` windows of `--horizons` horizons each, the
two paths alternating, every window ending in a device synchronise) and their spread.  `--check` compares the device's
head with the twin's through a deterministic actor, all H + 1 integers of it (see `check`).  `--collect-only` runs the
collect windows alone: the run to put under a kernel trace for the device time of ActorFeatures, PgxNetEval and
ActorSample."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import envpool_amd as envpool  # noqa: E402
from envpool_amd import torch_interop as ti  # noqa: E402
from envpool_amd.actor import BOX, Actor  # noqa: E402


class Collect:
    def __init__(self, task, n, horizon, seed, hidden, blocks):
        self.env = envpool.make(task, "gymnasium", num_envs=n, seed=seed)
        self.pool = self.env.device_pool
        self.dev = torch.device("cuda", self.pool.device)
        self.T = horizon
        self.ro = self.env.rollout(horizon=horizon, episodes=1 << 16)
        self.actor = Actor.random(self.env, hidden=hidden, blocks=blocks, seed=seed)
        self.ro.attach(self.actor, seed=seed)
        self.out = (torch.empty((horizon, n), dtype=torch.float32, device=self.dev),
                    torch.empty((horizon, n), dtype=torch.float32, device=self.dev))
        ti.rollout_reset_device(self.pool)
        self.values = ti.actor_view_device(self.pool)[1]

    def horizon(self):
        ti.rollout_collect_device(self.pool)
        ti.rollout_gae_device(self.pool, self.values, 0.99, 0.95, out=self.out)
        self.pool.rollout_next()


class Loop:
    """The parent commit's way: the policy is the caller's torch module, one Python turn per step."""

    def __init__(self, task, n, horizon, seed, hidden, blocks):
        self.env = envpool.make(task, "gymnasium", num_envs=n, seed=seed)
        self.pool = self.env.device_pool
        self.dev = dev = torch.device("cuda", self.pool.device)
        self.T, self.n = horizon, n
        self.pool.rollout_begin(horizon, 1 << 16, False)
        self.actor = Actor.random(self.env, hidden=hidden, blocks=blocks, seed=seed)
        self.m = self.actor.module().to(dev)
        self.box = self.actor.kind == BOX
        self.low = torch.tensor(self.actor.low, device=dev)
        self.high = torch.tensor(self.actor.high, device=dev)
        self.adtype = ti._torch_dtype(self.pool.action_dtype)
        self.values = torch.zeros((horizon + 1, n), dtype=torch.float32, device=dev)
        self.logp = torch.zeros((horizon, n), dtype=torch.float32, device=dev)
        self.out = (torch.empty((horizon, n), dtype=torch.float32, device=dev),
                    torch.empty((horizon, n), dtype=torch.float32, device=dev))
        self.obs = ti.rollout_reset_device(self.pool)["obs"]

    @torch.no_grad()
    def policy(self, obs):
        logits, value = self.m(obs)
        if self.box:
            z = torch.randn_like(logits)
            raw = logits + self.m.sigma * z
            logp = (-0.5 * z * z - torch.log(self.m.sigma) - 0.9189385).sum(dim=1)
            return torch.minimum(torch.maximum(raw, self.low), self.high).to(self.adtype).contiguous(), logp, value
        g = -torch.log(-torch.log(torch.rand_like(logits).clamp_(1e-7, 1 - 1e-7)))
        action = (logits + g).argmax(dim=1)
        logp = torch.log_softmax(logits, dim=1).gather(1, action.reshape(-1, 1)).reshape(-1)
        return action.to(self.adtype), logp, value

    def horizon(self):
        obs = self.obs
        for t in range(self.T):
            action, self.logp[t], self.values[t] = self.policy(obs)
            obs = ti.rollout_step_device(self.pool, action)["obs"]
        self.values[self.T] = self.policy(obs)[2]
        self.obs = obs
        ti.rollout_gae_device(self.pool, self.values, 0.99, 0.95, out=self.out)
        self.pool.rollout_next()


def window(path, horizons, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(horizons):
        path.horizon()
    torch.cuda.synchronize(dev)
    path.pool.synchronize()
    return time.perf_counter() - t0


def check(task, seed, hidden, blocks, n=4096):
    """A DETERMINISTIC actor on a pool of its own against its torch twin, on the observations of slot 0: the action and
    logp are then functions of every logit and the value of p[H], so all H + 1 head integers take part.
      value    the twin's p[H] * scale_v in float32, bit for bit
      action   Discrete: the twin's argmax;  Box: clamp(mu) with mu = p[j] * scale_p in float32, bit for bit in all H
      logp     the twin's float64 logp of that action, within the float32 rounding of the contract's own sum:
               (H + 8) 2^-23 max(1, |logp|) (Discrete), (5 H + 8) 2^-23 |logp| (Box; see tests/test_actor_host.py)"""
    env = envpool.make(task, "gymnasium", num_envs=n, seed=seed)
    pool = env.device_pool
    dev = torch.device("cuda", pool.device)
    ro = env.rollout(horizon=1)
    actor = Actor.random(env, hidden=hidden, blocks=blocks, seed=seed)
    ro.attach(actor, seed=seed, deterministic=True)
    ti.rollout_reset_device(pool)
    ti.rollout_collect_device(pool)
    view = ti.rollout_view_device(pool)
    logp, value = ti.actor_view_device(pool)
    m = actor.module().to(dev)
    with torch.no_grad():
        obs = view["obs"][0]
        logits, want_value = m(obs)
        h = actor.actions
        if actor.kind == BOX:
            low, high = torch.tensor(actor.low, device=dev), torch.tensor(actor.high, device=dev)
            want_action = torch.minimum(torch.maximum(logits, low), high).to(view["action"].dtype)
            want_logp = m.logp(obs, logits)  # z = 0
            tol = (5 * h + 8) * 2.0 ** -23 * float(want_logp.abs().max())
        else:
            want_action = logits.argmax(dim=1).to(view["action"].dtype)
            want_logp = m.logp(obs, want_action)
            tol = (h + 8) * 2.0 ** -23 * max(1.0, float(want_logp.abs().max()))
        out = {"rows": n, "value_equal": bool(torch.equal(value[0], want_value)),
               "action_equal": bool(torch.equal(view["action"][0].reshape(want_action.shape), want_action)),
               "logp_max_abs_diff": float((logp[0].to(torch.float64) - want_logp).abs().max()), "logp_bound": tol}
    out["logp_within_bound"] = out["logp_max_abs_diff"] <= tol
    ro.close()
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--horizons", type=int, default=8, help="horizons per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2, help="warm-up horizons per path")
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=1)
    ap.add_argument("--tasks", default="CartPole-v1,HalfCheetah-v4")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--collect-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_collect: no GPU; there is nothing to measure without one")
    for task in args.tasks.split(","):
        n, T = args.num_envs, args.horizon
        col = Collect(task, n, T, 1, args.hidden, args.blocks)
        dev = col.dev
        base = None if args.collect_only else Loop(task, n, T, 1, args.hidden, args.blocks)
        if args.check:
            print(json.dumps({"task": task, "check": check(task, 1, args.hidden, args.blocks)}), flush=True)
        for _ in range(args.warmup):
            col.horizon()
            if base is not None:
                base.horizon()
        tc, tb = [], []
        for _ in range(args.repeats):
            tc.append(window(col, args.horizons, dev))
            if base is not None:
                tb.append(window(base, args.horizons, dev))
        steps = args.horizons * T * n

        def rate(ts):
            return {"median": steps / float(np.median(ts)), "min": steps / max(ts), "max": steps / min(ts)}

        line = {"task": task, "num_envs": n, "horizon": T, "hidden": args.hidden, "blocks": args.blocks,
                "unit": "env-steps/s", "collect": rate(tc)}
        if base is not None:
            line["loop"] = rate(tb)
            line["collect_over_loop"] = line["collect"]["median"] / line["loop"]["median"]
        print(json.dumps(line), flush=True)
        col.ro.close()
        if base is not None:
            base.pool.rollout_end()


if __name__ == "__main__":
    main()
