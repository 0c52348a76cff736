"""Rollout collector on the device: twin pools with the same seed, one driven by `env.step`, the other by `ro.step`.
`ro.step` returns what `env.step` returns, bit for bit; `batch()`, `episodes()` and `gae()` equal the contract restated
in numpy (rollout_util.Model, fed the twin's `recv`), bit for bit; the moments stay within the summation bound of
numpy's float64 sums.  N = 257 is odd and more than one store block (64 rows) and moment group (256 rows); N = 1025
crosses the episode scan's block of 1024 envs."""
import numpy as np
import pytest

import envpool_amd as envpool
import rollout_util

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
N, T = 257, 7
TASKS = {
    "CartPole-v1": dict(max_episode_steps=3),   # every env truncates in the same step
    "CartPole-v1/long": {},                     # random play falls over within the window: term rows
    "Pendulum-v1": dict(max_episode_steps=5),
    "Taxi-v3": dict(max_episode_steps=4),
    "HalfCheetah-v4": dict(max_episode_steps=6),
    "MiniGrid-Empty-5x5-v0": dict(max_episode_steps=5),
    "Game2048-v1": dict(max_episode_steps=4),
}


def same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def make(case, n, seed=7, **kw):
    return envpool.make(case.split("/")[0], "gymnasium", num_envs=n, seed=seed, **dict(TASKS[case], **kw))


def actions(env, rng, n):
    dtype, shape = env._spec._action_spec[-1][0], tuple(env.action_space.shape)
    if hasattr(env.action_space, "n"):
        return rng.integers(0, env.action_space.n, n).astype(dtype)
    lo, hi = env.action_space.low, env.action_space.high
    return rng.uniform(lo, hi, (n, *shape)).astype(dtype)


def twin_step(twin, action):
    """The plain pool's step: (what env.step returns, the state dict recv returned)."""
    twin.send(action)
    rows = twin._recv()
    return twin._to(rows, False, True), dict(zip(twin._state_keys, rows))


def obs_dict(ro, b):
    return b.obs if isinstance(b.obs, dict) else {ro._names[0]: b.obs}


def check_moments(ro, model, rows):
    """rows: per moment component the float64 values of every obs row stored, [rows, comps]."""
    cnt, s1, s2 = ro.moments()
    total = len(rows)
    assert np.array_equal(cnt, np.full(rows.shape[1], float(total)))
    assert np.all(np.abs(s1 - rows.sum(axis=0)) <= total * U * np.abs(rows).sum(axis=0))
    assert np.all(np.abs(s2 - (rows * rows).sum(axis=0)) <= 2 * total * U * (rows * rows).sum(axis=0))
    assert same(np.stack([cnt, s1, s2]), model.mom)  # the same tree: the same bits


def run_twins(case, n=N, horizon=T, horizons=3, episodes=None, offset=0, moments=True, device=None, seed=7):
    kw = dict(env_id_offset=offset) if offset else {}
    twin = make(case, n, seed, **kw)
    env = make(case, n, seed, **(dict(kw, device=device) if device is not None else kw))
    episodes = 4 * n * horizon if episodes is None else episodes
    ro = env.rollout(horizon=horizon, episodes=episodes, moments=moments)
    pool = env._rollout()
    names = [pool.state_keys[i][0] for i in pool.rollout_obs_keys()]
    float_names = [nm for nm in names if np.dtype(dict((k, d) for k, d, _ in pool.state_keys)[nm]).kind == "f"]
    moments = moments and bool(float_names)
    model = rollout_util.Model(n, horizon, episodes, names, offset, moments)
    rng = np.random.default_rng(seed)
    out = dict(batches=[], episodes=[], gae=[], masks=[])
    first = ro.reset()
    twin._reset(twin.all_env_ids)
    rows = twin._recv()
    assert same(first, twin._to(rows, True, True))
    state = dict(zip(twin._state_keys, rows))
    model.reset(state)
    stored = [np.concatenate([np.asarray(state[k], np.float64).reshape(n, -1) for k in float_names], axis=1)] \
        if moments else []
    for h in range(horizons):
        for _ in range(horizon):
            a = actions(env, rng, n)
            got = ro.step(a)
            want, state = twin_step(twin, a)
            assert same(got, want), case
            model.step(a, state)
            if moments:
                stored.append(np.concatenate([np.asarray(state[k], np.float64).reshape(n, -1) for k in float_names],
                                             axis=1))
        b = ro.batch()
        mobs, maction, mreward, mterm, mtrunc, mmask = model.batch()
        assert same(obs_dict(ro, b), mobs), case
        assert same(b.action, maction) and same(b.reward, mreward)
        assert same(b.term.view(np.uint8), mterm) and same(b.trunc.view(np.uint8), mtrunc)
        assert same(b.mask.view(np.uint8), mmask), case
        values = rng.normal(0, 1, (horizon + 1, n)).astype(np.float32)
        adv, ret = ro.gae(values, 0.99, 0.95)
        madv, mret = model.gae(values, 0.99, 0.95)
        assert same(adv, madv) and same(ret, mret), case
        c = ro.counters
        assert (c["count"], c["finished"], c["dropped"], c["steps"]) == \
            (len(model.eps), model.finished, model.dropped, model.steps)
        if h != 1:  # (the second horizon's episodes stay in the buffer across next())
            eps = ro.episodes()
            assert same(tuple(eps), model.episodes()), case
            out["episodes"].append(eps)
        out["batches"].append(b)
        out["gae"].append((adv, ret))
        if moments:
            check_moments(ro, model, np.concatenate(stored))
        ro.next()
        model.next()
    if moments:
        out["moments"] = ro.moments()
    out["model"], out["env"], out["ro"], out["twin"] = model, env, ro, twin
    return out


def finish(out):
    out["ro"].close()
    out["env"].close()
    out["twin"].close()


@pytest.mark.parametrize("case", list(TASKS))
def test_twin_pools(case):
    out = run_twins(case)
    model = out["model"]
    if case == "CartPole-v1":
        # all 257 envs truncate in step 2; step 3 is the auto-reset row; step 6 = T - 1 truncates again, so the
        # carried flag masks t = 0 of the next horizon
        b0, b1 = out["batches"][0], out["batches"][1]
        assert b0.trunc[2].all() and not b0.mask[3].any() and b0.mask[[0, 1, 2, 4, 5, 6]].all()
        assert b0.trunc[6].all() and not b1.mask[0].any()
        assert model.finished == 5 * N and out["episodes"][0].length.tolist() == [3] * (2 * N)
    if case == "CartPole-v1/long":
        assert any(b.term.any() for b in out["batches"])
    if case not in ("CartPole-v1/long", "Game2048-v1"):  # (a random game of 2048 outlasts the window and never truncates)
        assert any(b.trunc.any() for b in out["batches"]), "the window holds no episode end"
    finish(out)


@pytest.mark.parametrize("n", [1, 1025])
def test_one_env_and_more_than_a_scan_block(n):
    out = run_twins("CartPole-v1", n=n, horizons=1)
    assert out["model"].finished == 2 * n
    assert out["episodes"][0].env_id.tolist() == list(range(n)) * 2
    finish(out)


def test_env_id_offset():
    out = run_twins("CartPole-v1", n=65, offset=3, horizons=1)
    assert out["episodes"][0].env_id[:65].tolist() == list(range(3, 68))
    finish(out)


def test_episode_buffer_overflow_is_counted():
    out = run_twins("CartPole-v1", n=65, episodes=4, horizons=3)
    model = out["model"]
    assert model.dropped > 0 and out["ro"].counters["dropped"] == model.dropped
    assert all(len(e.env_id) <= 4 for e in out["episodes"])
    finish(out)


def test_sharded_pool_equals_the_unsharded_pool():
    """device=[0, 0]: two shards with a collector each; the arrays are the unsharded pool's (the twin is unsharded)."""
    out = run_twins("CartPole-v1", n=130, device=[0, 0], moments=False)
    finish(out)
    out = run_twins("Pendulum-v1", n=130, device=[0, 0], moments=False, episodes=40)
    assert out["model"].dropped > 0
    finish(out)


def test_identical_runs_give_identical_moment_bits():
    a = run_twins("HalfCheetah-v4", horizons=1)
    b = run_twins("HalfCheetah-v4", horizons=1)
    assert same(a["moments"], b["moments"])
    finish(a)
    finish(b)


def test_what_a_pool_refuses():
    env = make("CartPole-v1", 8)
    ro = env.rollout(horizon=2, episodes=4)
    with pytest.raises(ValueError, match="not been reset"):
        ro.step(np.zeros(8, np.int32))
    ro.reset()
    with pytest.raises(ValueError, match="open rollout collector"):  # a forced reset in mid-rollout
        env.reset(np.array([1, 2], np.int32))
    with pytest.raises(ValueError, match="open rollout collector"):
        env.reset()
    with pytest.raises(ValueError, match="whole horizon"):
        ro.gae(np.zeros((3, 8), np.float32))
    ro.step(np.zeros(8, np.int32))
    ro.step(np.zeros(8, np.int32))
    with pytest.raises(ValueError, match="horizon of 2 steps is full"):
        ro.step(np.zeros(8, np.int32))
    with pytest.raises(ValueError, match="values"):
        ro.gae(np.zeros((3, 8), np.float64))
    with pytest.raises(ValueError, match="no moments"):
        ro.moments()
    ro.close()
    with pytest.raises(ValueError, match="closed"):
        ro.step(np.zeros(8, np.int32))
    env.reset()  # the pool is the caller's again
    with pytest.raises(ValueError, match="horizon"):
        env.rollout(horizon=0)
    env.close()
    env = envpool.make("CartPole-v1", "gymnasium", num_envs=8, batch_size=4)
    with pytest.raises(ValueError, match="async"):
        env.rollout(horizon=2)
    env.close()
    env = envpool.make("TicTacToe-v1", "gymnasium", num_envs=4)
    with pytest.raises(RuntimeError, match="rollout not implemented for this environment"):
        env.rollout(horizon=2)
    env.close()


def test_device_forms_equal_the_numpy_forms():
    torch = pytest.importorskip("torch")
    from envpool_amd import torch_interop as ti

    n, horizon = 257, 7
    a_env, b_env = make("HalfCheetah-v4", n), make("HalfCheetah-v4", n)
    ro = a_env.rollout(horizon=horizon, episodes=64, moments=True)
    pool = b_env._rollout()
    pool.rollout_begin(horizon, 64, True)
    dev = torch.device("cuda", pool.device)
    rng = np.random.default_rng(3)
    first = ro.reset()
    t0 = ti.rollout_reset_device(pool)
    assert same(first[0], t0["obs"].cpu().numpy())
    for _ in range(horizon):
        a = actions(a_env, rng, n)
        got = ro.step(a)
        out = ti.rollout_step_device(pool, torch.from_numpy(np.ascontiguousarray(a, pool.action_dtype)).to(dev))
        assert same(got[0], out["obs"].cpu().numpy()) and same(got[1], out["reward"].cpu().numpy().reshape(-1))
        assert same(got[2] | got[3], out["done"].cpu().numpy())
    b = ro.batch()
    view = ti.rollout_view_device(pool)
    assert same(b.obs, view["obs"].cpu().numpy()) and same(b.action, view["action"].cpu().numpy())
    assert same(b.reward, view["reward"].cpu().numpy())
    for name in ("term", "trunc", "mask"):
        assert same(getattr(b, name).view(np.uint8), view[name].cpu().numpy())
    values = rng.normal(0, 1, (horizon + 1, n)).astype(np.float32)
    adv, ret = ro.gae(values, 0.99, 0.95)
    dadv, dret = ti.rollout_gae_device(pool, torch.from_numpy(values).to(dev), 0.99, 0.95)
    assert same(adv, dadv.cpu().numpy()) and same(ret, dret.cpu().numpy())
    arrays, count = ti.rollout_episodes_view_device(pool)
    k = int(count.cpu()[0])
    eps = ro.episodes()
    assert k == len(eps.env_id) and k > 0
    assert same(tuple(eps), tuple(x[:k].cpu().numpy() for x in arrays))
    assert same(np.stack(ro.moments()), ti.rollout_moments_device(pool).cpu().numpy())
    pool.rollout_end()
    ro.close()
    a_env.close()
    b_env.close()
