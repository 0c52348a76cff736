"""Jumanji board puzzles on the MI355X: every reference fixture (tests/golden/jumanji_*.npz, made by the
reference itself) replayed bit-exact -- every state key, and the hidden state through get_state -- through
DevicePool, through make(..., "gymnasium") / make(..., "dm") and the `Jumanji/` alias, a sharded pool, as
the last rows of a 65536-env pool, in async mode, on the device path, and from set_state; plus Snake's
bounded fruit placement raising from recv."""
import numpy as np
import pytest

import envpool_amd as envpool
from envpool_amd.core.device_pool import DevicePool
from jumanji_util import NAMES, PREFIX, config, extra_config, fixture, params, state_keys, task_id

pytestmark = pytest.mark.gpu

COMMON = ["reward", "done", "trunc", "elapsed_step", "step_type", "discount", "info:env_id"]
# one fixture per puzzle for the slower routes
ONE_EACH = ["Game2048-v1", "Minesweeper-v0__mines", "SlidingTilePuzzle-v0__puzzle", "RubiksCube-v0__scramble1",
            "RubiksCube-partly-scrambled-v0", "Snake-v1", "Maze-v0__on_target"]


def _row_keys(name):
    return {k: k.replace(":", "__") for k in COMMON + state_keys(name) if k != "info:env_id"}


def _pool(name, g, n=None, **kw):
    n = n or g["actions"].shape[1]
    native, p = params(name)
    p.update(kw.pop("params", {}))
    return DevicePool(native, n, seed=int(g["seed"]), max_episode_steps=config(name)["max_episode_steps"],
                      params=p, **kw)


def _check(out, g, t, name, rows=slice(None)):
    for k, gk in _row_keys(name).items():
        a = np.asarray(out[k])[rows].reshape(g[gk][t].shape)
        assert np.array_equal(a, g[gk][t]), (name, t, k)


def _get(tree, key):
    for p in key.split(":", 1)[1].split("."):
        tree = tree[p] if isinstance(tree, dict) else getattr(tree, p)
    return np.asarray(tree)


@pytest.mark.parametrize("name", NAMES)
def test_device_pool_replays_fixture(name):
    g = fixture(name)
    steps, n = g["actions"].shape[:2]
    ids = np.arange(n, dtype=np.int32)
    pool = _pool(name, g)
    pool.reset(ids)
    for t in range(steps + 1):
        _check(pool.recv_dict(), g, t, name)
        st = pool.get_state()
        assert np.array_equal(st[:, 2:].astype(np.int64), g["hidden"][t]), (name, t)
        assert np.array_equal(st[:, 0].astype(np.int64), g["elapsed_step"][t]), (name, t)
        if t < steps:
            pool.send(ids, g["actions"][t])
    pool.close()


@pytest.mark.parametrize("name", NAMES)
def test_make_gymnasium_dm_and_alias_replay_fixture(name):
    g = fixture(name)
    steps, n = g["actions"].shape[:2]
    obs_keys = [k for k in state_keys(name) if k.startswith("obs:")]
    for route, tid in (("gymnasium", task_id(name)), ("dm", task_id(name)), ("gymnasium", f"Jumanji/{task_id(name)}")):
        env = envpool.make(tid, route, num_envs=n, seed=int(g["seed"]), **extra_config(name))
        first = env.reset()
        obs = first[0] if route == "gymnasium" else first.observation
        for k in obs_keys:
            assert np.array_equal(_get(obs, k), g[k.replace(":", "__")][0]), (name, route, k)
        for t in range(steps):
            if route == "gymnasium":
                obs, rew, term, trunc, info = env.step(g["actions"][t])
                assert np.array_equal(term, g["done"][t + 1] & ~g["trunc"][t + 1]), (name, t)
                assert np.array_equal(trunc, g["trunc"][t + 1]), (name, t)
                assert np.array_equal(info["elapsed_step"], g["elapsed_step"][t + 1]), (name, t)
            else:
                ts = env.step(g["actions"][t])
                obs, rew = ts.observation, ts.reward
                assert np.array_equal(ts.step_type, g["step_type"][t + 1]), (name, t)
                assert np.array_equal(ts.discount, g["discount"][t + 1]), (name, t)
            assert np.array_equal(rew, g["reward"][t + 1]), (name, route, t)
            for k in obs_keys:
                assert np.array_equal(_get(obs, k), g[k.replace(":", "__")][t + 1]), (name, route, t, k)
        env.close()


@pytest.mark.parametrize("name", ONE_EACH)
def test_sharded_pool_replays_fixture(name):
    """device=[0, 0]: two shards of 4 envs (env_id_offset 0 and 4, each its own DevicePool and error word)
    replay the fixture's 8 envs like one pool."""
    g = fixture(name)
    steps, n = g["actions"].shape[:2]
    env = envpool.make(task_id(name), "gymnasium", num_envs=n, seed=int(g["seed"]), device=[0, 0],
                       **extra_config(name))
    obs_keys = [k for k in state_keys(name) if k.startswith("obs:")]
    obs, info = env.reset()
    assert np.array_equal(info["env_id"], np.arange(n))
    for t in range(steps):
        obs, rew, term, trunc, info = env.step(g["actions"][t])
        assert np.array_equal(rew, g["reward"][t + 1]), (name, t)
        assert np.array_equal(term | trunc, g["done"][t + 1]), (name, t)
        for k in obs_keys:
            assert np.array_equal(_get(obs, k), g[k.replace(":", "__")][t + 1]), (name, t, k)
    env.close()


@pytest.mark.parametrize("name", ONE_EACH)
def test_fixture_envs_as_last_rows_of_a_big_pool(name):
    g = fixture(name)
    steps, m = g["actions"].shape[:2]
    steps = min(steps, 320)
    n = 65536
    seeds = np.arange(n, dtype=np.int64) * 7 + 11
    seeds[n - m:] = int(g["seed"]) + np.arange(m)
    pool = _pool(name, g, n=n, env_seed=[int(s) for s in seeds])
    ids = np.arange(n, dtype=np.int32)
    rng = np.random.default_rng(5)
    pool.reset(ids)
    rows = slice(n - m, n)
    shape = g["actions"].shape[2:]
    for t in range(steps + 1):
        _check(pool.recv_dict(), g, t, name, rows)
        if t < steps:
            act = rng.integers(-1, 11, (n, *shape)).astype(np.int32)
            act[rows] = g["actions"][t]
            pool.send(ids, act)
    pool.close()


@pytest.mark.parametrize("name", ONE_EACH)
def test_async_mode_matches_per_env(name):
    g = fixture(name)
    steps, n = g["actions"].shape[:2]
    pool = _pool(name, g, batch_size=n // 2)
    keys = _row_keys(name)
    t_env = np.zeros(n, np.int64)
    pool.reset(np.arange(n, dtype=np.int32))
    for _ in range(2 * 120):
        out = pool.recv_dict()
        eids = out["info:env_id"].astype(np.int64)
        for r, e in enumerate(eids):
            for k, gk in keys.items():
                assert np.array_equal(np.asarray(out[k])[r], g[gk][t_env[e], e]), (name, e, t_env[e], k)
        pool.send(eids.astype(np.int32), g["actions"][t_env[eids], eids])
        t_env[eids] += 1
    assert t_env.min() > 50
    pool.close()


@pytest.mark.parametrize("name", ["Minesweeper-v0", "RubiksCube-v0", "Snake-v1", "Game2048-v1"])
def test_device_path_bit_identical_to_numpy_path(name):
    """step_device (actions resident on the GPU, Minesweeper's and RubiksCube's several elements per env
    included) against send / recv of the same actions."""
    import torch

    from envpool_amd.torch_interop import recv_device_tensors, send_device_tensors

    g = fixture(name)
    n = 1000
    host, dev = _pool(name, g, n=n), _pool(name, g, n=n)
    ids = np.arange(n, dtype=np.int32)
    rng = np.random.default_rng(3)
    shape = g["actions"].shape[2:]
    host.reset(ids)
    dev.reset(ids)
    a = host.recv_dict()
    b = {k: v.cpu().numpy() for k, v in recv_device_tensors(dev).items()}
    for t in range(150):
        for k in a:
            assert np.array_equal(np.asarray(a[k]), b[k].reshape(np.asarray(a[k]).shape)), (name, t, k)
        act = rng.integers(-1, 11, (n, *shape)).astype(np.int32)
        host.send(ids, act)
        a = host.recv_dict()
        send_device_tensors(dev, torch.as_tensor(act, device="cuda:0"), torch.as_tensor(ids, device="cuda:0"))
        b = {k: v.cpu().numpy() for k, v in recv_device_tensors(dev).items()}
    host.close()
    dev.close()


@pytest.mark.parametrize("name", ONE_EACH)
def test_set_state_round_trip_and_teacher_forcing(name):
    g = fixture(name)
    steps, n = g["actions"].shape[:2]
    steps = min(steps, 320)
    ids = np.arange(n, dtype=np.int32)
    pool = _pool(name, g)
    pool.reset(ids)
    pool.recv_dict()
    st = pool.get_state()
    other = st.copy()
    other[:, 2:] = st[::-1, 2:]
    pool.set_state(other)
    assert np.array_equal(pool.get_state()[:, 2:], other[:, 2:])
    pool.set_state(st)
    assert np.array_equal(pool.get_state(), st)
    # teacher forcing: before every step, the state the reference had there is set
    for t in range(steps):
        s = pool.get_state()
        s[:, 0] = g["elapsed_step"][t]
        s[:, 1] = g["done"][t]
        s[:, 2:] = g["hidden"][t]
        pool.set_state(s)
        pool.send(ids, g["actions"][t])
        out = pool.recv_dict()
        # (a row that resets draws from the generator, whose position set_state does not carry)
        stepped = ~g["done"][t]
        for k, gk in _row_keys(name).items():
            assert np.array_equal(np.asarray(out[k])[stepped], g[gk][t + 1][stepped]), (name, t, k)
    pool.close()


def test_snake_exhausted_fruit_bound_raises_from_recv():
    """snake_max_tries = 1: about 1 in 144 first fruit draws lands on the head, so some of 4096 first resets
    run out; recv raises (the reference would spin).  The default bound resets the same seeds cleanly."""
    n = 4096
    _, p = params("Snake-v1")
    pool = DevicePool("Snake", n, seed=0, max_episode_steps=4000, params=dict(p, snake_max_tries=1.0))
    pool.reset(np.arange(n, dtype=np.int32))
    with pytest.raises(RuntimeError, match="snake_max_tries"):
        pool.recv_dict()
    pool.close()
    pool = DevicePool("Snake", n, seed=0, max_episode_steps=4000, params=p)
    pool.reset(np.arange(n, dtype=np.int32))
    out = pool.recv_dict()
    assert (out["elapsed_step"] == 0).all()
    assert (out["obs:grid"][..., 1].reshape(n, -1).sum(1) == 1).all()  # one head per env
    pool.close()


def test_make_snake_alias_small_pool():
    env = envpool.make("Jumanji/Snake-v1", "gymnasium", num_envs=4)
    obs, info = env.reset()
    assert obs["grid"].shape == (4, 12, 12, 5) and obs["grid"].dtype == np.float32
    obs, rew, term, trunc, info = env.step(np.zeros(4, np.int32))
    assert rew.shape == (4,)
    env.close()
