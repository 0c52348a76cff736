"""MiniGrid on the MI355X at configs outside the 30 registered ids: the option cases of
tests/golden/minigrid_option_cases.json (other grid sides, non-square DistShift, fixed and random starts, every
river count up to the 16 of size 19, wall-type LavaGap, 0..8 obstacles, short max_episode_steps), each a fixture
made by the reference itself (tests/golden/make_minigrid_golden.py --options) and reproduced on the host by
tests/test_minigrid_host.py.  Replayed bit for bit through DevicePool, as rows on both sides of a block boundary,
and through make(<registered id>, ..., **kwargs); plus the configs the engine refuses."""
import numpy as np
import pytest

import envpool_amd as envpool
from envpool_amd.core.device_pool import DevicePool
from minigrid_util import OPTION_CASES, option_config, option_fixture, option_kwargs, option_params
from test_gpu_minigrid import HEAD, ROW_KEYS

pytestmark = pytest.mark.gpu

# one case per task
PER_TASK = ["empty19_rand", "doorkey19", "dist12x9", "cross19n16", "gap19w", "dyn16n8"]


def _pool(case, g, n=None, **kw):
    return DevicePool("MiniGrid", n or g["actions"].shape[1], seed=int(g["seed"]),
                      max_episode_steps=option_config(case)["max_episode_steps"], params=option_params(case), **kw)


def _check_rows(out, g, t, rows, ctx):
    for k, gk in ROW_KEYS.items():
        a = np.asarray(out[k])[rows].reshape(g[gk][t].shape)
        assert np.array_equal(a, g[gk][t]), (ctx, t, k)


def _check_state(st, g, t, ctx):
    assert np.array_equal(st[:, HEAD:].astype(np.uint8), g["grid"][t]), (ctx, t, "grid")
    assert np.array_equal(st[:, 2:5].astype(np.int32), g["agent"][t]), (ctx, t, "agent")
    assert np.array_equal(st[:, 5:8].astype(np.int32), g["carrying"][t]), (ctx, t, "carrying")
    assert np.array_equal(st[:, 8:24].astype(np.int32), g["obstacles"][t]), (ctx, t, "obstacles")


@pytest.mark.parametrize("case", OPTION_CASES)
def test_device_pool_replays_option_fixture(case):
    g = option_fixture(case)
    steps, n = g["actions"].shape
    ids = np.arange(n, dtype=np.int32)
    pool = _pool(case, g)
    assert pool.state_dim() == HEAD + 3 * int(g["width"]) * int(g["height"])
    pool.reset(ids)
    for t in range(steps + 1):
        out = pool.recv_dict()
        _check_rows(out, g, t, slice(None), case)
        assert np.array_equal(np.asarray(out["info:env_id"]).ravel(), ids), (case, t)
        _check_state(pool.get_state(), g, t, case)
        if t < steps:
            pool.send(ids, g["actions"][t])
    pool.close()


@pytest.mark.parametrize("case", PER_TASK)
def test_fixture_envs_across_a_block_boundary(case):
    """300 envs = one full 256-thread block and a partial one of 44 rows; the fixture's envs are rows 252..259, four
    in each block, so their images go through both blocks' LDS staging and cooperative copy."""
    g = option_fixture(case)
    m = g["actions"].shape[1]
    steps = min(g["actions"].shape[0], 150)
    n, first = 300, 252
    seeds = np.arange(n, dtype=np.int64) * 7 + 11
    seeds[first:first + m] = int(g["seed"]) + np.arange(m)
    pool = _pool(case, g, n=n, env_seed=[int(s) for s in seeds])
    ids = np.arange(n, dtype=np.int32)
    mine = np.arange(first, first + m, dtype=np.int32)
    rows = slice(first, first + m)
    rng = np.random.default_rng(5)
    pool.reset(ids)
    for t in range(steps + 1):
        out = pool.recv_dict()
        _check_rows(out, g, t, rows, case)
        assert np.array_equal(np.asarray(out["info:env_id"]).ravel(), ids), (case, t)
        _check_state(pool.get_state(mine), g, t, case)
        if t < steps:
            act = rng.integers(0, 3, n).astype(np.int32)
            act[rows] = g["actions"][t]
            pool.send(ids, act)
    pool.close()


def _gymnasium_replay(case, pair):
    g = option_fixture(case)
    steps, n = g["actions"].shape
    task_id, kw = option_kwargs(case, pair)
    env = envpool.make(task_id, "gymnasium", num_envs=n, seed=int(g["seed"]), **kw)
    obs, info = env.reset()
    assert np.array_equal(obs["image"], g["obs__image"][0]), case
    assert np.array_equal(obs["direction"], g["obs__direction"][0]), case
    assert np.array_equal(obs["mission"], g["obs__mission"][0]), case
    assert np.array_equal(info["agent_pos"], g["info__agent_pos"][0]), case
    for t in range(steps):
        obs, rew, term, trunc, info = env.step(g["actions"][t])
        assert np.array_equal(obs["image"], g["obs__image"][t + 1]), (case, t)
        assert np.array_equal(obs["direction"], g["obs__direction"][t + 1]), (case, t)
        assert np.array_equal(obs["mission"], g["obs__mission"][t + 1]), (case, t)
        assert np.array_equal(rew, g["reward"][t + 1]), (case, t)
        assert np.array_equal(term, g["done"][t + 1] & ~g["trunc"][t + 1]), (case, t)
        assert np.array_equal(trunc, g["trunc"][t + 1]), (case, t)
        assert np.array_equal(info["agent_pos"], g["info__agent_pos"][t + 1]), (case, t)
        assert np.array_equal(info["elapsed_step"], g["elapsed_step"][t + 1]), (case, t)
    env.close()


@pytest.mark.parametrize("case", PER_TASK)
def test_make_gymnasium_with_kwargs_replays_option_fixture(case):
    _gymnasium_replay(case, tuple)  # (empty19_rand: agent_start_pos as a tuple)


def test_make_dm_with_kwargs_replays_option_fixture():
    case = "empty19_rand"
    g = option_fixture(case)
    steps, n = g["actions"].shape
    task_id, kw = option_kwargs(case, list)  # agent_start_pos as a list
    env = envpool.make(task_id, "dm", num_envs=n, seed=int(g["seed"]), **kw)
    ts = env.reset()
    assert np.array_equal(ts.observation.image, g["obs__image"][0])
    for t in range(steps):
        ts = env.step(g["actions"][t])
        assert np.array_equal(ts.observation.image, g["obs__image"][t + 1]), t
        assert np.array_equal(ts.observation.direction, g["obs__direction"][t + 1]), t
        assert np.array_equal(ts.observation.mission, g["obs__mission"][t + 1]), t
        assert np.array_equal(ts.reward, g["reward"][t + 1]), t
        assert np.array_equal(ts.step_type, g["step_type"][t + 1]), t
        assert np.array_equal(np.asarray(ts.discount).ravel(), g["discount"][t + 1].ravel()), t
    env.close()


EMPTY, DOORKEY, DIST = "MiniGrid-Empty-8x8-v0", "MiniGrid-DoorKey-8x8-v0", "MiniGrid-DistShift1-v0"
CROSS, DYN = "MiniGrid-LavaCrossingS9N1-v0", "MiniGrid-Dynamic-Obstacles-8x8-v0"


@pytest.mark.parametrize("task_id, kw, key", [
    (CROSS, dict(size=8), "size"),                          # even: the reference CHECK-fails
    (CROSS, dict(size=9, num_crossings=0), "num_crossings"),
    (CROSS, dict(size=9, num_crossings=7), "num_crossings"),    # rivers + 1: the reference puts lava on the top wall
    (CROSS, dict(size=19, num_crossings=17), "num_crossings"),  # one more than the 16 nibbles hold
    (EMPTY, dict(size=4), "size"),
    (EMPTY, dict(size=20), "size"),
    (DOORKEY, dict(size=4), "size"),
    (DOORKEY, dict(size=20), "size"),
    (DIST, dict(width=20), "width"),
    (DIST, dict(height=4, strip2_row=2), "height"),
    (DIST, dict(strip2_row=0), "strip2_row"),
    (DIST, dict(height=7, strip2_row=6), "strip2_row"),     # height - 1: the bottom wall
    (EMPTY, dict(agent_start_pos=(0, 3)), "agent_start_pos"),   # on the left wall
    (EMPTY, dict(agent_start_pos=(3, 7)), "agent_start_pos"),   # on the bottom wall of the 8 x 8 grid
    (DIST, dict(agent_start_pos=(8, 1)), "agent_start_pos"),    # on the right wall of the 9 x 7 grid
    (EMPTY, dict(agent_start_dir=4), "agent_start_dir"),
    (DYN, dict(size=17), "size"),
    (DYN, dict(n_obstacles=-1), "n_obstacles"),
    (DYN, dict(size=16, n_obstacles=9), "n_obstacles"),     # 9 <= size / 2 + 1 is not clamped: over the packing's 8
])
def test_unsupported_option_raises_at_construction(task_id, kw, key):
    """Refused on the host when the pool is made, by a message that names the key; nothing is launched."""
    with pytest.raises(ValueError, match=key):
        envpool.make(task_id, "gymnasium", num_envs=8, **kw)
