"""Rollout actor with memory on the device.  `actor_eval(memory=)` and `collect()` equal the numpy restatements --
features, the cell (actor_memory_util), the trunk's head and the sample -- bit for bit, the collector's states included.
The tasks give the (F, M) pairs a pool can reach: F = 3 with M = 32 for both kinds; F = 20 and 17 with M = 64; F = 244
and 376 with M = 512, where the cell's tile has 32 rows instead of 64; F = 3 and 17 put most blocks' feature span off a
dword.  (F = 19 and F = 512 exist in no registered task; the host test has the cell by the book there.)"""
import numpy as np
import pytest

import actor_memory_util as mu
import actor_util as au
import envpool_amd as envpool
from envpool_amd.actor import Actor
from envpool_amd.pgx.net import Net

pytestmark = pytest.mark.gpu

EVAL = [("Blackjack-v1", 32), ("Pendulum-v1", 32), ("Game2048-v1", 64), ("HalfCheetah-v4", 64),
        ("MiniGrid-Empty-5x5-v0", 512), ("Humanoid-v4", 512)]
SEED = 2**40 + 5


def open_ro(task, n, memory, horizon, seed=7):
    env = envpool.make(task, "gymnasium", num_envs=n, seed=seed)
    ro = env.rollout(horizon=horizon, episodes=4 * n * horizon)
    a = Actor.random(env, hidden=32, blocks=1, seed=2, memory=memory)
    # (the logits scaled down by 16: the noise decides, not one action of a random net)
    net = Net(a.net.obs_shape, a.actions, 32, 1, a.net.layers, a.net.scale_p / 16, a.net.scale_v)
    actor = Actor(net, a.kind, a.lo, a.scale, a.sigma, a.low, a.high, cell=a.cell)
    ro.attach(actor, seed=SEED)
    return env, ro, actor


def slot_of(ro, obs, t):
    return [obs[k][t] for k in ro._names] if isinstance(obs, dict) else [obs[t]]


def restate(actor, obs, h, ids, step):
    out = mu.cell(actor.cell, au.features(obs, actor.lo, actor.scale), h)
    p = au.head(actor.net.layers, actor.net.blocks, out)
    sp, sv = actor.net.scale_p, actor.net.scale_v
    if actor.kind == 0:
        return (*au.discrete(p, sp, sv, SEED, ids, step, False), out)
    return (*au.box(p, sp, sv, actor.sigma, actor.low, actor.high, SEED, ids, step, False), out)


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return np.array_equal(got.reshape(want.shape), want.astype(got.dtype))


@pytest.mark.parametrize("task,memory", EVAL)
def test_actor_eval_equals_the_restatement(task, memory):
    env, ro, actor = open_ro(task, 200, memory, 4)
    ro.reset(), ro.collect(2)
    obs = slot_of(ro, ro.batch().obs, 2)
    before = ro.memory()
    rng = np.random.default_rng(memory)
    for rows in (1, 63, 65, 200):  # the tile's edges and a partial last block, for both tile heights
        h = rng.integers(0, 128, (rows, memory)).astype(np.uint8)
        rows_obs = [o[:rows] for o in obs]
        ids = env.all_env_ids[:rows]
        got = ro.actor_eval(dict(zip(ro._names, rows_obs)) if len(obs) > 1 else rows_obs[0], ids, step=12, memory=h)
        want = restate(actor, rows_obs, h, ids, 12)
        for g, w, name in zip(got, want, ("action", "logp", "value", "memory")):
            assert same(g, w), (task, rows, name)
        assert len(np.unique(got[3])) > 8, "the cell must not saturate"
    assert all(np.array_equal(a, b) for a, b in zip(before, ro.memory())), "actor_eval touches no collector state"
    with pytest.raises(ValueError, match="memory"):
        ro.actor_eval(obs[0] if len(obs) == 1 else dict(zip(ro._names, obs)))
    ro.close(), env.close()


@pytest.mark.parametrize("task", ["Catch-v0", "Pendulum-v1"])
def test_collect_equals_the_restatement(task):
    torch = pytest.importorskip("torch")
    from envpool_amd import torch_interop as ti

    n, horizon, m = 96, 24, 32
    env, ro, actor = open_ro(task, n, m, horizon)
    env_b, ro_b, _ = open_ro(task, n, m, horizon)
    ro.reset(), ro_b.reset()
    assert not ro.memory()[0].any() and not ro.memory()[1].any()
    ro.collect()
    ro_b.collect(10), ro_b.collect(14)
    b, ids = ro.batch(), env.all_env_ids
    for x, y in zip(b[1:] + ro.memory(), ro_b.batch()[1:] + ro_b.memory()):
        assert np.array_equal(x, y), "collect(10) then collect(14) is collect(24)"
    assert (not b.mask.all()) == (task == "Catch-v0"), "Catch's episodes end inside the horizon, Pendulum's do not"

    def replay(b, h, step0, steps):
        for t in range(steps):
            a, lp, v, out = restate(actor, slot_of(ro, b.obs, t), h, ids, step0 + t)
            assert same(b.action[t], a) and same(b.logp[t], lp) and same(b.value[t], v), (task, t)
            h = np.where(b.mask[t][:, None], out, 0).astype(np.uint8)  # the state rule
        assert same(b.value[steps], restate(actor, slot_of(ro, b.obs, steps), h, ids, step0 + steps)[2])
        return h

    h = replay(b, np.zeros((n, m), np.uint8), 0, horizon)
    h0, h_now = ro.memory()
    assert not h0.any() and np.array_equal(h_now, h) and h.any()
    ro.next()
    assert all(np.array_equal(x, h) for x in ro.memory()), "after next() h0 is the old h"
    ro.collect(3)  # across the horizon's edge: slot 0 is evaluated with the carried state
    assert np.array_equal(replay(ro.batch(), h, horizon, 3), ro.memory()[1]) and np.array_equal(ro.memory()[0], h)
    # the torch forms: the views alias the states, the device eval equals the host's and refuses a misaligned state
    pool = env._rollout()
    assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(ti.actor_memory_view_device(pool), ro.memory()))
    dev = torch.device("cuda", pool.device)
    d_obs = ti.rollout_view_device(pool)[ro._names[0]][3].contiguous()
    d_ids = torch.tensor(ids, dtype=torch.int32, device=dev)
    got = ti.actor_eval_device(pool, d_obs, d_ids, 5, memory=torch.tensor(h, device=dev))
    assert all(same(g.cpu().numpy(), w) for g, w in zip(got, ro.actor_eval(d_obs.cpu().numpy(), ids, 5, memory=h)))
    with pytest.raises(ValueError, match="16-byte aligned"):
        odd = torch.zeros(n * m + 1, dtype=torch.uint8, device=dev)[1:].reshape(n, m)
        ti.actor_eval_device(pool, d_obs, d_ids, 5, memory=odd)
    ro.reset()
    assert not ro.memory()[0].any() and not ro.memory()[1].any()
    for x in (ro, ro_b, env, env_b):
        x.close()
