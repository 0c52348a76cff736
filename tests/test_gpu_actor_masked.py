"""The masked head of the rollout actor (kind 2) on the device against the numpy restatement (actor_masked_util): the
sample kernels through `actor_eval` on caller observations, exactly; the loss kernel within the header's bound; collect
and fit on Minesweeper and Game2048 pools end to end."""
import numpy as np
import pytest

import actor_masked_util as mu
import actor_util as au
import envpool_amd as envpool
import pgx_train_util as TU
import ppo_trainer_util as U
from envpool_amd import actor_trainer as T
from envpool_amd.actor import Actor
from envpool_amd.pgx.net import Net

pytestmark = pytest.mark.gpu
ROWS, CLIP, VW, EW = 70, 0.2, 0.5, 0.01  # two full blocks of 32 rows and a tail of 6


def softer(a):
    """The same actor with logits scaled down by 16, so that the noise decides."""
    net = Net(a.net.obs_shape, a.actions, a.net.hidden, a.net.blocks, a.net.layers, a.net.scale_p / 16, a.net.scale_v)
    return Actor(net, 2, a.lo, a.scale, mask0=a.mask0, nvec=a.nvec[:a.components])


# H = 100 as (10, 10) is Minesweeper's own space; the others live in the 147 uint8 components of MiniGrid's image key
# (components 1 .. 147 of F = 244), the mask from component 4 on, on a pool whose action row is one int32
@pytest.mark.parametrize("h", [2, 9, 64, 65, 100, 127])
@pytest.mark.parametrize("deterministic", [False, True])
def test_sample(h, deterministic):
    rng = np.random.default_rng(h)
    if h == 100:
        env = envpool.make("Minesweeper-v0", "gymnasium", num_envs=8, seed=1)
        actor = softer(Actor.random(env, hidden=32, seed=h, mask=True))
        obs = [rng.integers(-1, 9, (ROWS, 10, 10)).astype(np.int32), mu.masks(rng, ROWS, h).reshape(ROWS, 10, 10),
               np.full(ROWS, 10, np.int32), rng.integers(0, 90, ROWS).astype(np.int32)]
        mask = obs[1]
    else:
        env = envpool.make("MiniGrid-Empty-5x5-v0", "gymnasium", num_envs=8, seed=1)
        space = dict(features=244, kind=2, actions=h, mask0=4, nvec=[h], low=[], high=[], obs_low=np.zeros(244),
                     obs_high=np.full(244, 10.0))
        actor = softer(Actor.random(space, hidden=32, seed=h))
        obs = [rng.integers(0, 4, ROWS).astype(np.int32), rng.integers(0, 11, (ROWS, 7, 7, 3)).astype(np.uint8),
               rng.integers(0, 11, (ROWS, 96)).astype(np.uint8)]
        mask = obs[1].reshape(ROWS, 147)[:, 3:3 + h]
        mask[:] = mask.clip(1) * mu.masks(rng, ROWS, h)   # any value that is not 0 counts
    ro = env.rollout(horizon=2)
    pool = env._rollout()
    ids = (np.arange(ROWS, dtype=np.int32) * 5) % 8
    pool.actor_begin(actor, 2**40 + 5, deterministic, h)
    action, logp, value = pool.actor_eval(obs, ids, 12)
    legal = mu.legal_of(mask)
    p = au.head(actor.net.layers, 1, au.features(obs, actor.lo, actor.scale))
    wa, wl, wv = mu.sample(p, legal, actor.net.scale_p, actor.net.scale_v, 2**40 + 5, ids, 12, deterministic)
    assert np.array_equal(action.reshape(ROWS, -1), np.stack(np.unravel_index(wa, actor.nvec[:actor.components]), axis=1))
    assert np.array_equal(logp.view(np.uint32), wl.view(np.uint32)) and np.array_equal(value, wv)
    assert legal[np.arange(ROWS), wa].all() and not legal.all() and len(np.unique(wa)) > 1
    if deterministic:
        assert np.array_equal(wa, np.where(legal, p[:, :h], -2**31).argmax(axis=1))
    if h != 100:  # rows 2 (all legal) and 3 (none legal) against a kind-0 actor of the same net, seed and step
        pool.actor_begin(Actor(actor.net, 0, actor.lo, actor.scale), 2**40 + 5, deterministic, h)
        da, dl, dv = pool.actor_eval(obs, ids, 12)
        assert np.array_equal(da.ravel()[2:4], action.ravel()[2:4])
        assert np.array_equal(dl[2:4].view(np.uint32), logp[2:4].view(np.uint32)) and np.array_equal(dv, value)
    ro.close(), env.close()


@pytest.mark.parametrize("h,nvec", [(2, [2]), (65, [65]), (100, [10, 10]), (127, [127])])
def test_loss(h, nvec):
    f = 18
    space = dict(features=f, kind=2, actions=h, mask0=-1, nvec=nvec, low=[], high=[], obs_low=np.zeros(f), obs_high=np.ones(f))
    actor = Actor.random(space, hidden=32, blocks=0, seed=h)
    feat = TU.rows_of(f, ROWS, h, binary=False)
    p = TU.forward_np(actor.net, feat)[1].astype(np.int32)
    sp, sv = actor.net.scale_p, actor.net.scale_v
    rng = np.random.default_rng(h)
    m = mu.masks(rng, ROWS, h)
    legal = mu.legal_of(m)
    action = np.array([rng.choice(np.flatnonzero(row)) for row in legal], np.int32)
    _, _, adv, ret, mask = U.batch(0, p, 4, sp)   # (row 1 has mask 0)
    lp = mu.loss(p, legal, action, np.zeros(ROWS, np.float32), adv, ret, mask, sp, 1.0, CLIP, VW, 0.0)["lp"]
    d = np.array([-0.5, 0.5, -0.1, 0.1, 0.5, -0.5, 0.1, -0.1])[np.arange(ROWS) % 8]  # far from log(0.8), log(1.2)
    logp = (lp - d).astype(np.float32)
    want = mu.loss(p, legal, action, logp, adv, ret, mask, sp, sv, CLIP, VW, EW)
    U.check_draw(0, want, mask)
    tr = actor.trainer(lr=0.0, clip_ratio=CLIP, value_weight=VW, entropy_weight=EW, max_rows=ROWS)
    tr.step(feat, action, logp, adv, ret, mask.astype(bool), legal=m)   # (bool rows: packed by the call)
    assert np.array_equal(tr.read(T.P), p)
    dp, stats = tr.read(T.DP), tr.stats()
    row, row_mag, unmasked, n = U.stats_row(want, mask, ROWS)
    checks = [U.within(dp, want["dp"], want["mag"]), U.within(stats[0, :5], row, row_mag)]
    print(f"worst err / bound = {max(w for _, w in checks):.3g}")
    assert all(ok for ok, _ in checks) and want["dp"].any()
    assert stats[0, 6] == unmasked and stats[0, 7] == n
    assert not dp[:, :h][~legal].any() and not dp[mask == 0].any()   # exactly 0
    tr.close()


@pytest.mark.parametrize("task", ["Minesweeper-v0", "Game2048-v1"])
def test_collect_and_fit(task):
    n, horizon, batch, seed = 64, 8, 256, 5
    env = envpool.make(task, "gymnasium", num_envs=n, seed=7)
    ro = env.rollout(horizon=horizon, episodes=4 * n * horizon)
    actor = softer(Actor.random(env, hidden=32, seed=2, mask=True))
    ro.attach(actor, seed=9)
    ro.reset()
    ro.collect()
    b = ro.batch()
    tn = n * horizon
    obs = [b.obs[k][:horizon].reshape(tn, -1) for k in ro._names]
    raw = obs[ro._names.index("obs:action_mask")] != 0
    comp = b.action.reshape(tn, -1)
    flat = comp[:, 0] * 10 + comp[:, 1] if task.startswith("Mine") else comp[:, 0]   # (row, col) = divmod(flat, 10)
    some = raw.any(axis=1)   # (an all-false mask: the slot after a done)
    assert some.sum() > tn // 2 and raw[some, flat[some]].all() and len(np.unique(flat)) > 1
    adv, ret = ro.gae(None, 0.99, 0.95)
    cnt, mean, std = U.adv_stats(adv, b.mask)
    options = dict(optimizer="adam", lr=1.0, clip=0.5)
    tr = actor.trainer(seed=seed, max_rows=batch, **options)
    twin = actor.trainer(seed=seed, max_rows=batch, **options)   # stepped from numpy, minibatch by minibatch
    layers = len(actor.net.layers)
    rule = U.Rule([w for w, _, _ in actor.net.layers] + [c for _, c, _ in actor.net.layers], **options)
    tr.fit(ro, epochs=1, batch=batch, gamma=0.99, lam=0.95)
    for step in range(tn // batch):
        idx = np.array([U.permute(seed, 0, step * batch + j, tn) for j in range(batch)])
        parts = (actor.features_of([x[idx] for x in obs]), flat[idx].astype(np.int32), b.logp.ravel()[idx],
                 U.adv_normalize(adv.ravel()[idx], mean, std), ret.ravel()[idx], b.mask.ravel()[idx])
        twin.step(*parts, legal=mu.words(raw[idx]))
        rule.step([twin.read(T.GRADIENT, i) for i in range(2 * layers)])
    for part, want in zip((T.FEATURES, T.ACTION, T.LOGP, T.ADV, T.RET, T.MASK), parts):   # the last minibatch
        assert np.array_equal(tr.read(T.BATCH, part), want), part
    assert np.array_equal(tr.read(T.BATCH, T.LEGAL), mu.words(raw[idx]))
    for i in range(2 * layers):
        assert np.array_equal(tr.read(T.MASTER, i), rule.master[i]), i
        assert np.array_equal(tr.read(T.QUANTISED, i), rule.quantised(i, i < layers)), i
    new = tr.actor()
    assert (new.kind, new.mask0, list(new.nvec)) == (2, actor.mask0, list(actor.nvec))
    assert any((l[0] != o[0]).any() for l, o in zip(new.net.layers, actor.net.layers))
    tr.close(), twin.close(), ro.close(), env.close()
