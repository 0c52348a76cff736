"""MiniGrid navigation family on the MI355X: every reference fixture (tests/golden/minigrid_*.npz, made by
the reference itself) replayed bit-exact through DevicePool, through make(..., "gymnasium") and
make(..., "dm"), as the last rows of a 65536-env pool, in async mode, on the device path, and from
set_state; plus the bounded rejection sampling's error path."""
import numpy as np
import pytest

import envpool_amd as envpool
from envpool_amd.core.device_pool import DevicePool
from minigrid_util import IDS, config, fixture, params

pytestmark = pytest.mark.gpu

HEAD = 24  # MiniGrid get_state: cur_step, done, x, y, dir, carried (3), obstacles (16), then the grid
ROW_KEYS = {"obs:direction": "obs__direction", "obs:image": "obs__image", "obs:mission": "obs__mission",
            "info:agent_pos": "info__agent_pos", "info:mission_id": "info__mission_id", "reward": "reward",
            "done": "done", "trunc": "trunc", "elapsed_step": "elapsed_step", "step_type": "step_type",
            "discount": "discount"}


def _pool(task_id, g, n=None, **kw):
    n = n or g["actions"].shape[1]
    conf = config(task_id)
    return DevicePool("MiniGrid", n, seed=int(g["seed"]), max_episode_steps=conf["max_episode_steps"],
                      params=params(task_id), **kw)


def _check(out, g, t, rows=slice(None), ctx=""):
    for k, gk in ROW_KEYS.items():
        a = np.asarray(out[k])[rows].reshape(g[gk][t].shape)
        assert np.array_equal(a, g[gk][t]), (ctx, t, k)


def _grid_of(state, g):
    return state[:, HEAD:].astype(np.uint8)


@pytest.mark.parametrize("task_id", IDS)
def test_device_pool_replays_fixture(task_id):
    g = fixture(task_id)
    n = g["actions"].shape[1]
    ids = np.arange(n, dtype=np.int32)
    pool = _pool(task_id, g)
    pool.reset(ids)
    for t in range(g["actions"].shape[0] + 1):
        out = pool.recv_dict()
        _check(out, g, t, ctx=task_id)
        st = pool.get_state()
        assert np.array_equal(_grid_of(st, g), g["grid"][t]), (task_id, t)
        assert np.array_equal(st[:, 2:5].astype(np.int32), g["agent"][t]), (task_id, t)
        assert np.array_equal(st[:, 5:8].astype(np.int32), g["carrying"][t]), (task_id, t)
        assert np.array_equal(st[:, 8:24].astype(np.int32), g["obstacles"][t]), (task_id, t)
        if t < g["actions"].shape[0]:
            pool.send(ids, g["actions"][t])
    pool.close()


@pytest.mark.parametrize("task_id", IDS)
def test_make_gymnasium_and_dm_replay_fixture(task_id):
    from envpool_amd.minigrid import decode_mission

    g = fixture(task_id)
    n = g["actions"].shape[1]
    env = envpool.make(task_id, "gymnasium", num_envs=n, seed=int(g["seed"]))
    obs, info = env.reset()
    assert np.array_equal(obs["image"], g["obs__image"][0])
    assert decode_mission(obs["mission"][0]) == decode_mission(g["obs__mission"][0, 0])
    for t in range(g["actions"].shape[0]):
        obs, rew, term, trunc, info = env.step(g["actions"][t])
        assert np.array_equal(obs["image"], g["obs__image"][t + 1]), (task_id, t)
        assert np.array_equal(obs["direction"], g["obs__direction"][t + 1]), (task_id, t)
        assert np.array_equal(rew, g["reward"][t + 1]), (task_id, t)
        assert np.array_equal(np.logical_or(term, trunc), g["done"][t + 1]), (task_id, t)
        assert np.array_equal(trunc, g["trunc"][t + 1]), (task_id, t)
        assert np.array_equal(info["agent_pos"], g["info__agent_pos"][t + 1]), (task_id, t)
    env.close()
    env = envpool.make(task_id, "dm", num_envs=n, seed=int(g["seed"]))
    ts = env.reset()
    assert np.array_equal(ts.observation.image, g["obs__image"][0])
    for t in range(g["actions"].shape[0]):
        ts = env.step(g["actions"][t])
        assert np.array_equal(ts.observation.image, g["obs__image"][t + 1]), (task_id, t)
        assert np.array_equal(ts.reward, g["reward"][t + 1]), (task_id, t)
        assert np.array_equal(ts.step_type, g["step_type"][t + 1]), (task_id, t)
    env.close()


@pytest.mark.parametrize("task_id", ["MiniGrid-FourRooms-v0", "MiniGrid-Dynamic-Obstacles-8x8-v0",
                                     "MiniGrid-LavaCrossingS11N5-v0"])
def test_fixture_envs_as_last_rows_of_a_big_pool(task_id):
    g = fixture(task_id)
    steps, m = g["actions"].shape
    n = 65536
    seeds = np.arange(n, dtype=np.int64) * 7 + 11
    seeds[n - m:] = int(g["seed"]) + np.arange(m)
    pool = _pool(task_id, g, n=n, env_seed=[int(s) for s in seeds])
    ids = np.arange(n, dtype=np.int32)
    rng = np.random.default_rng(5)
    pool.reset(ids)
    rows = slice(n - m, n)
    for t in range(steps + 1):
        out = pool.recv_dict()
        _check(out, g, t, rows, task_id)
        if t < steps:
            act = rng.integers(0, 3, n).astype(np.int32)
            act[rows] = g["actions"][t]
            pool.send(ids, act)
    pool.close()


@pytest.mark.parametrize("task_id", ["MiniGrid-DoorKey-6x6-v0", "MiniGrid-Dynamic-Obstacles-Random-6x6-v0",
                                     "MiniGrid-LavaCrossingS9N2-v0"])
def test_sharded_pool_replays_fixture(task_id):
    """device=[0, 0]: two shards of 4 envs (env_id_offset 0 and 4, each its own DevicePool and error word) replay
    the fixture's 8 envs like one pool (tests/test_gpu_sharded.py lists the one GPU twice the same way)."""
    g = fixture(task_id)
    n = g["actions"].shape[1]
    env = envpool.make(task_id, "gymnasium", num_envs=n, seed=int(g["seed"]), device=[0, 0])
    obs, info = env.reset()
    assert np.array_equal(obs["image"], g["obs__image"][0])
    assert np.array_equal(info["env_id"], np.arange(n))
    for t in range(g["actions"].shape[0]):
        obs, rew, term, trunc, info = env.step(g["actions"][t])
        assert np.array_equal(obs["image"], g["obs__image"][t + 1]), (task_id, t)
        assert np.array_equal(obs["direction"], g["obs__direction"][t + 1]), (task_id, t)
        assert np.array_equal(obs["mission"], g["obs__mission"][t + 1]), (task_id, t)
        assert np.array_equal(rew, g["reward"][t + 1]), (task_id, t)
        assert np.array_equal(term, g["done"][t + 1] & ~g["trunc"][t + 1]), (task_id, t)
        assert np.array_equal(trunc, g["trunc"][t + 1]), (task_id, t)
        assert np.array_equal(info["agent_pos"], g["info__agent_pos"][t + 1]), (task_id, t)
        assert np.array_equal(info["elapsed_step"], g["elapsed_step"][t + 1]), (task_id, t)
    env.close()


@pytest.mark.parametrize("task_id", ["MiniGrid-DoorKey-8x8-v0", "MiniGrid-Dynamic-Obstacles-6x6-v0"])
def test_async_mode_matches_per_env(task_id):
    g = fixture(task_id)
    steps, n = g["actions"].shape
    pool = _pool(task_id, g, batch_size=n // 2)
    t_env = np.zeros(n, np.int64)
    pool.reset(np.arange(n, dtype=np.int32))
    for _ in range(2 * 120):
        out = pool.recv_dict()
        eids = out["info:env_id"].astype(np.int64)
        for r, e in enumerate(eids):
            t = t_env[e]
            for k, gk in ROW_KEYS.items():
                assert np.array_equal(np.asarray(out[k])[r], g[gk][t, e]), (task_id, e, t, k)
        pool.send(eids.astype(np.int32), g["actions"][t_env[eids], eids])
        t_env[eids] += 1
    assert t_env.min() > 50
    pool.close()


def test_device_path_bit_identical_to_numpy_path():
    import torch

    from envpool_amd.torch_interop import recv_device_tensors, send_device_tensors

    task_id = "MiniGrid-Dynamic-Obstacles-16x16-v0"
    g = fixture(task_id)
    n = 1000
    host, dev = _pool(task_id, g, n=n), _pool(task_id, g, n=n)
    ids = np.arange(n, dtype=np.int32)
    rng = np.random.default_rng(3)
    host.reset(ids)
    dev.reset(ids)
    a = host.recv_dict()
    b = {k: v.cpu().numpy() for k, v in recv_device_tensors(dev).items()}
    for t in range(120):
        for k in a:
            assert np.array_equal(np.asarray(a[k]), b[k].reshape(np.asarray(a[k]).shape)), (t, k)
        act = rng.integers(0, 3, n).astype(np.int32)
        host.send(ids, act)
        a = host.recv_dict()
        send_device_tensors(dev, torch.as_tensor(act, device="cuda:0"), torch.as_tensor(ids, device="cuda:0"))
        b = {k: v.cpu().numpy() for k, v in recv_device_tensors(dev).items()}
    host.close()
    dev.close()


@pytest.mark.parametrize("task_id", ["MiniGrid-DoorKey-5x5-v0", "MiniGrid-Dynamic-Obstacles-8x8-v0",
                                     "MiniGrid-FourRooms-v0"])
def test_set_state_round_trip_and_teacher_forcing(task_id):
    g = fixture(task_id)
    steps, n = g["actions"].shape
    ids = np.arange(n, dtype=np.int32)
    pool = _pool(task_id, g)
    pool.reset(ids)
    pool.recv_dict()
    st = pool.get_state()
    # round trip: a state written back reads back the same
    other = st.copy()
    other[:, HEAD:] = st[::-1, HEAD:]
    pool.set_state(other)
    assert np.array_equal(pool.get_state(), other)
    pool.set_state(st)
    assert np.array_equal(pool.get_state(), st)
    # teacher forcing: before every step, the state the reference had there (its DebugState) is set
    for t in range(steps):
        s = pool.get_state()
        s[:, HEAD:] = g["grid"][t]
        s[:, 2:5] = g["agent"][t]
        s[:, 5:8] = g["carrying"][t]
        s[:, 8:24] = g["obstacles"][t]
        s[:, 0] = g["elapsed_step"][t]
        s[:, 1] = g["done"][t]
        pool.set_state(s)
        pool.send(ids, g["actions"][t])
        _check(pool.recv_dict(), g, t + 1, ctx=task_id)
    pool.close()


def test_exhausted_rejection_bound_raises_from_recv():
    """minigrid_max_tries = 1 on FourRooms: the first reset's placement runs out of tries for some envs.
    recv raises (the reference would throw in a worker or, with its unbounded default, spin)."""
    task_id = "MiniGrid-FourRooms-v0"
    n = 256
    p = dict(params(task_id), minigrid_max_tries=1.0)
    pool = DevicePool("MiniGrid", n, seed=0, max_episode_steps=100, params=p)
    pool.reset(np.arange(n, dtype=np.int32))
    with pytest.raises(RuntimeError, match="minigrid_max_tries"):
        pool.recv_dict()
    pool.close()
    # the default bound: the same seeds reset fine
    pool = DevicePool("MiniGrid", n, seed=0, max_episode_steps=100, params=params(task_id))
    pool.reset(np.arange(n, dtype=np.int32))
    out = pool.recv_dict()
    assert (out["elapsed_step"] == 0).all()
    pool.close()
