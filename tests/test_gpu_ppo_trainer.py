"""The rollout actor's PPO trainer on the device (csrc/ppo_trainer.hip, `actor.trainer(...)`) against the float64 numpy
restatements of its contract (tests/ppo_trainer_util.py): the loss of both heads, update and re-quantising with the
trained sigma, `fit` on a collector's buffers, and the refusals."""
import numpy as np
import pytest

import actor_util as au
import envpool_amd as envpool
import pgx_train_util as TU
import ppo_trainer_util as U
from envpool_amd import actor_trainer as T
from envpool_amd.actor import Actor

pytestmark = pytest.mark.gpu
F, CLIP, VW, EW = 18, 0.2, 0.5, 0.01
STEPS = {"CartPole-v1": 3, "Pendulum-v1": 3, "Taxi-v3": 4}  # max_episode_steps: masked rows inside a horizon


def actor_of(kind, h, seed):
    space = dict(features=F, kind=kind, actions=h, low=-np.ones(h * kind, np.float32), high=np.ones(h * kind, np.float32),
                 obs_low=np.zeros(F), obs_high=np.ones(F))
    a = Actor.random(space, hidden=32, blocks=0, seed=seed)
    a.sigma = np.random.default_rng(seed).uniform(0.3, 1.5, h * kind).astype(np.float32)
    return a


# H + 1 below, at and above a wave's 64 lanes; rows: one, past a block, past four blocks
@pytest.mark.parametrize("rows", [1, 65, 130])
@pytest.mark.parametrize("kind,h", [(0, 2), (0, 63), (0, 127), (1, 1), (1, 6), (1, 17)])
def test_loss(kind, h, rows):
    actor = actor_of(kind, h, seed=h)
    feat = TU.rows_of(F, rows, rows, binary=False)
    p = TU.forward_np(actor.net, feat)[1].astype(np.int32)
    sp, sv = actor.net.scale_p, actor.net.scale_v
    sigma = actor.sigma if kind == U.BOX else None
    action, logp, adv, ret, mask = U.batch(kind, p, h, sp, sigma)
    want = U.loss(kind, p, action, logp, adv, ret, mask, sp, sv, CLIP, VW, EW, sigma)
    if rows > 1:
        U.check_draw(kind, want, mask, action)
    tr = actor.trainer(lr=0.0, clip_ratio=CLIP, value_weight=VW, entropy_weight=EW, max_rows=rows)
    tr.step(feat, action, logp, adv, ret, mask.astype(bool))
    assert np.array_equal(tr.read(T.P), p)
    dp, stats = tr.read(T.DP), tr.stats()
    checks = [U.within(dp, want["dp"], want["mag"])]
    row, row_mag, unmasked, n = U.stats_row(want, mask, rows)
    checks.append(U.within(stats[0, :5], row, row_mag))
    if kind == U.BOX:
        checks.append(U.within(tr.read(T.GRADIENT, tr.sigma_layer), want["dsigma"].sum(axis=0),
                               want["dsigma_mag"].sum(axis=0)))
    print(f"worst err / bound = {max(w for _, w in checks):.3g}")
    assert all(ok for ok, _ in checks) and want["dp"].any()
    assert stats.shape == (1, 8) and stats[0, 6] == unmasked and stats[0, 7] == n
    assert not dp[mask == 0].any()
    tr.close()


@pytest.mark.parametrize("kind", [0, 1], ids=["discrete", "box"])
@pytest.mark.parametrize("optimizer,clipped", [("sgd", False), ("adam", False), ("sgd", True)])
def test_update(kind, optimizer, clipped):
    h = 6
    actor = actor_of(kind, h, seed=3)
    net = actor.net
    n = len(net.layers)
    feat = TU.rows_of(F, 40, 2, binary=False)
    p = TU.forward_np(net, feat)[1].astype(np.int32)
    action, logp, adv, ret, mask = U.batch(kind, p, 4, net.scale_p, actor.sigma if kind else None)
    if kind:  # component 0 at its mean, every row pushing the same way: its sigma has to shrink
        action[:, 0] = p[:, 0].astype(np.float32) * np.float32(net.scale_p)
        logp = U.loss(kind, p, action, logp, adv, ret, mask, net.scale_p, 1.0, CLIP, VW, 0.0, actor.sigma)["lp"]
        logp, adv = logp.astype(np.float32), np.abs(adv)
    args = (feat, action, logp, adv, ret, mask)
    arrays = lambda tr, what: [tr.read(what, i) for i in range(2 * n + kind)]
    probe = actor.trainer(lr=0.0, max_rows=64)  # the first gradient: what the step sizes are chosen by
    probe.step(*args)
    first, norm = arrays(probe, T.GRADIENT), probe.stats()[0, 5]
    probe.close()
    clip = norm / 2 if clipped else 0.0
    top = max(np.abs(g).max() for g in first[:n])
    # the largest first change of a weight is 300 (adam: all about 30): past the clamp, smaller ones cross roundings;
    # and far enough for sigma 0 (gradient above 0) to pass the floor
    lr = 30.0 if optimizer == "adam" else 300.0 / (top * (0.5 if clipped else 1.0))
    if kind and optimizer == "sgd":
        assert first[2 * n][0] > 0
        lr = max(lr, 4.0 * actor.sigma[0] / first[2 * n][0])
    options = dict(optimizer=optimizer, lr=lr, momentum=0.9, weight_decay=1e-4 * top, clip=clip, eps=1e-6 * top)
    tr = actor.trainer(max_rows=64, **options)
    masters = [w for w, _, _ in net.layers] + [b for _, b, _ in net.layers] + ([actor.sigma] if kind else [])
    rule = U.Rule(masters, **options)
    floored = False  # (sigma 0 reaches the floor in the first step; from there its gradient turns)
    for step in range(2):  # (the second step reads the state the first wrote)
        tr.step(*args)
        got_norm = rule.step(arrays(tr, T.GRADIENT))
        assert got_norm == tr.stats()[0, 5] and (not clipped or step > 0 or got_norm > clip)  # (the clip bites)
        for i in range(2 * n + kind):
            assert np.array_equal(tr.read(T.MASTER, i), rule.master[i]), (step, i)
            assert np.array_equal(tr.read(T.STATE1, i), rule.s1[i]), (step, i)
            assert optimizer == "sgd" or np.array_equal(tr.read(T.STATE2, i), rule.s2[i]), (step, i)
            want = rule.quantised(i, i < n) if i < 2 * n else np.maximum(rule.master[i], U.SIGMA_MIN).astype(np.float32)
            assert np.array_equal(tr.read(T.QUANTISED, i), want), (step, i)
            floored = floored or (i == 2 * n and want[0] == np.float32(U.SIGMA_MIN))
    moved = [rule.quantised(i, True) != net.layers[i][0] for i in range(n)]
    assert any((np.abs(rule.master[i]) > 127.5).any() for i in range(n)) and any(m.any() for m in moved)
    assert floored == bool(kind)
    tr.close()


def collected(task, n=48, horizon=5):
    env = envpool.make(task, "gymnasium", num_envs=n, seed=7, max_episode_steps=STEPS[task])
    ro = env.rollout(horizon=horizon, episodes=4 * n * horizon)
    actor = Actor.random(env, hidden=32, blocks=1, seed=2)
    ro.attach(actor, seed=9)
    ro.reset()
    return env, ro, actor


# T N = 240 is no power of two (cycle walking), 240 // 64 leaves a tail, N is no multiple of 32; Taxi's id is int32, F = 1
@pytest.mark.parametrize("task", ["CartPole-v1", "Pendulum-v1", "Taxi-v3"])
def test_fit(task):
    env, ro, actor = collected(task)
    ro.collect()
    b = ro.batch()
    adv, ret = ro.gae(None, 0.99, 0.95)
    obs = [b.obs[k] for k in ro._names] if isinstance(b.obs, dict) else [b.obs]
    flat = [o[:5].reshape(240, -1) for o in obs]
    cnt, mean, std = U.adv_stats(adv, b.mask)
    assert cnt < 240  # (a masked row inside the horizon)
    tr = actor.trainer(lr=1.0, seed=5, max_rows=128)
    for epochs, batch, epoch, first in ((1, 128, 0, 0), (2, 64, 2, 128)):  # the last minibatch: (epoch, first position)
        tr.fit(ro, epochs=epochs, batch=batch, gamma=0.99, lam=0.95)
        assert tr.stats().shape == (epochs * (240 // batch), 8) and (tr.stats()[:, 7] == batch).all()
        idx = np.array([U.permute(5, epoch, first + j, 240) for j in range(batch)])
        assert np.array_equal(tr.read(T.BATCH, T.ADV_STATS), [cnt, mean, std])
        assert np.array_equal(tr.read(T.BATCH, T.FEATURES), actor.features_of([x[idx] for x in flat]))
        assert np.array_equal(tr.read(T.BATCH, T.ACTION), b.action.reshape(240, -1)[idx].reshape(
            (batch, actor.actions) if actor.kind else (batch,)).astype(np.float32 if actor.kind else np.int32))
        assert np.array_equal(tr.read(T.BATCH, T.LOGP), b.logp.ravel()[idx])
        assert np.array_equal(tr.read(T.BATCH, T.ADV), U.adv_normalize(adv.ravel()[idx], mean, std))
        assert np.array_equal(tr.read(T.BATCH, T.RET), ret.ravel()[idx])
        assert np.array_equal(tr.read(T.BATCH, T.MASK), b.mask.ravel()[idx])
        assert tr.stats()[-1, 6] == b.mask.ravel()[idx].sum()
    # tr.actor() is the twin of the quantised arrays, and the collector evaluates it as such
    new = tr.actor()
    assert any((l[0] != o[0]).any() for l, o in zip(new.net.layers, actor.net.layers))
    ro.attach(new, seed=1, deterministic=True)
    rows = [o[0] for o in obs]
    ids = np.arange(48, dtype=np.int32)
    got = ro.actor_eval(dict(zip(ro._names, rows)) if len(rows) > 1 else rows[0], ids, step=3)
    p = au.head(new.net.layers, 1, new.features_of(rows))
    if new.kind:
        want = au.box(p, new.net.scale_p, new.net.scale_v, new.sigma, new.low, new.high, 1, ids, 3, True)
    else:
        want = au.discrete(p, new.net.scale_p, new.net.scale_v, 1, ids, 3, True)
    assert all(np.array_equal(np.asarray(x).reshape(np.shape(y)), y) for x, y in zip(got, want))
    tr.close(), ro.close()


@pytest.mark.parametrize("bad", ["no actor", "not full", "batch", "closed", "kind"])
def test_refusals(bad):
    env, ro, actor = collected("CartPole-v1", n=8, horizon=2)
    tr = actor.trainer(max_rows=64)
    other = None
    if bad == "no actor":
        ro.close()
        ro = env.rollout(horizon=2)
        ro.reset()
    elif bad == "closed":
        tr.close()
    elif bad == "kind":
        other = Actor.random(envpool.make_spec("Pendulum-v1"), hidden=32).trainer(max_rows=64)
    if bad != "not full" and bad != "no actor":
        ro.collect()
    with pytest.raises(ValueError):
        (other or tr).fit(ro, epochs=1, batch=17 if bad == "batch" else 8)
    tr.close(), ro.close()
    if other is not None:
        other.close()
