"""PGX board games on the MI355X: every reference fixture (tests/golden/pgx_*.npz, made by the reference itself)
replayed bit-exact -- every state key, per-player keys as 2 rows per env, and the hidden state through get_state --
through DevicePool, make(..., "gymnasium") / make(..., "dm"), async mode, the device path, as the last rows of a
65536-env pool and through a sharded pool; plus the multi-player checks of a live pool."""
import numpy as np
import pytest

import envpool_amd as envpool
from envpool_amd.core.device_pool import DevicePool
from pgx_util import ACTIONS, KEYS, NAMES, PER_PLAYER, check_rows, fixture, game, hidden, task_id

pytestmark = pytest.mark.gpu

ONE_EACH = ["TicTacToe-v1", "ConnectFour-v1", "Hex-v1", "Othello-v1"]


def _pool(name, g, n=None, **kw):
    n = n or g["actions"].shape[1]
    return DevicePool(game(name), n, seed=int(g["seed"]), max_episode_steps=int(g["max_episode_steps"]), **kw)


def _kw(name, g):
    kw = dict(seed=int(g["seed"]))
    if int(g["max_episode_steps"]) != 2**31 - 1:
        kw["max_episode_steps"] = int(g["max_episode_steps"])
    return kw


@pytest.mark.parametrize("name", NAMES)
def test_device_pool_replays_fixture(name):
    g = fixture(name)
    steps, n = g["actions"].shape
    ids = np.arange(n, dtype=np.int32)
    want_hidden = hidden(g)
    pool = _pool(name, g)
    assert pool.players == 2
    pool.reset(ids)
    for t in range(steps + 1):
        check_rows(pool.recv_dict(), g, t, name)
        st = pool.get_state()
        assert np.array_equal(st[:, 2:].astype(np.int64), want_hidden[t]), (name, t)
        assert np.array_equal(st[:, 0].astype(np.int64), g["elapsed_step"][t]), (name, t)
        if t < steps:
            pool.send(ids, g["actions"][t])
    pool.close()


@pytest.mark.parametrize("name", NAMES)
def test_make_gymnasium_and_dm_replay_fixture(name):
    g = fixture(name)
    steps, n = g["actions"].shape
    for route in ("gymnasium", "dm"):
        env = envpool.make(task_id(name), route, num_envs=n, **_kw(name, g))
        first = env.reset()
        obs = first[0] if route == "gymnasium" else first.observation.obs
        assert np.array_equal(obs, g["obs"][0].reshape(2 * n, *g["obs"].shape[3:])), (name, route)
        for t in range(steps):
            if route == "gymnasium":
                obs, rew, term, trunc, info = env.step(g["actions"][t])
                assert term.shape == (n,) and rew.shape == (2 * n,)
                assert np.array_equal(term, g["done"][t + 1] & ~g["trunc"][t + 1]), (name, t)
                assert np.array_equal(trunc, g["trunc"][t + 1]), (name, t)
                assert np.array_equal(info["players"]["id"], g["info:players.id"][t + 1].ravel()), (name, t)
                assert np.array_equal(info["players"]["env_id"], g["info:players.env_id"][t + 1].ravel()), (name, t)
                assert np.array_equal(info["board"], g["info:board"][t + 1]), (name, t)
                assert np.array_equal(info["legal_action_mask"], g["info:legal_action_mask"][t + 1]), (name, t)
                assert np.array_equal(info["current_player"], g["info:current_player"][t + 1]), (name, t)
            else:
                ts = env.step(g["actions"][t])
                obs, rew = ts.observation.obs, ts.reward
                assert ts.step_type.shape == (n,) and ts.discount.shape == (2 * n,)
                assert np.array_equal(ts.step_type, g["step_type"][t + 1]), (name, t)
                assert np.array_equal(ts.discount, g["discount"][t + 1].ravel()), (name, t)
                assert np.array_equal(ts.observation.players.id, g["info:players.id"][t + 1].ravel()), (name, t)
                assert np.array_equal(ts.observation.legal_action_mask,
                                      g["info:legal_action_mask"][t + 1]), (name, t)
            assert np.array_equal(rew, g["reward"][t + 1].ravel()), (name, route, t)
            assert np.array_equal(obs, g["obs"][t + 1].reshape(2 * n, *g["obs"].shape[3:])), (name, route, t)
        env.close()


@pytest.mark.parametrize("name", ONE_EACH)
def test_async_mode_matches_per_env(name):
    g = fixture(name)
    steps, n = g["actions"].shape
    pool = _pool(name, g, batch_size=n // 2)
    t_env = np.zeros(n, np.int64)
    pool.reset(np.arange(n, dtype=np.int32))
    while t_env.min() < min(steps, 120):
        out = pool.recv_dict()
        eids = out["info:env_id"].astype(np.int64)
        assert len(eids) == n // 2
        for k in KEYS:
            got = np.asarray(out[k])
            if k in PER_PLAYER:
                assert got.shape[0] == 2 * len(eids)
                got = got.reshape(len(eids), 2, *got.shape[1:])
            for r, e in enumerate(eids):
                assert np.array_equal(got[r], g[k][t_env[e], e]), (name, e, t_env[e], k)
        act = g["actions"][np.minimum(t_env[eids], steps - 1), eids]
        pool.send(eids.astype(np.int32), act)
        t_env[eids] += 1
    pool.close()


@pytest.mark.parametrize("name", NAMES)
def test_device_path_replays_fixture(name):
    """Actions resident on the GPU (send_device_tensors / recv_device_tensors): every key, per-player keys as
    [2 k, ...] device views."""
    import torch

    from envpool_amd.torch_interop import recv_device_tensors, send_device_tensors

    g = fixture(name)
    steps, n = g["actions"].shape
    pool = _pool(name, g)
    ids = torch.arange(n, dtype=torch.int32, device="cuda:0")
    send_device_tensors(pool, None, ids)
    for t in range(steps + 1):
        out = {k: v.cpu().numpy() for k, v in recv_device_tensors(pool).items()}
        check_rows(out, g, t, name)
        if t < steps:
            send_device_tensors(pool, torch.as_tensor(g["actions"][t], device="cuda:0"), ids)
    pool.close()


@pytest.mark.parametrize("name", ONE_EACH)
def test_device_path_bit_identical_to_numpy_path(name):
    """step_device with legal actions drawn on the GPU ((mask * rand).argmax) against send / recv of the same
    actions, 4096 envs."""
    import torch

    from envpool_amd.torch_interop import recv_device_tensors, send_device_tensors

    g = fixture(name)
    n = 4096
    host, dev = _pool(name, g, n=n), _pool(name, g, n=n)
    ids = np.arange(n, dtype=np.int32)
    gen = torch.Generator(device="cuda:0").manual_seed(7)
    host.reset(ids)
    send_device_tensors(dev, None, torch.as_tensor(ids, device="cuda:0"))
    for t in range(200):
        a = host.recv_dict()
        b = {k: v.cpu().numpy() for k, v in recv_device_tensors(dev).items()}
        for k in KEYS:
            assert np.array_equal(np.asarray(a[k]), b[k]), (name, t, k)
        mask = torch.as_tensor(b["info:legal_action_mask"], device="cuda:0")
        act = (mask.float() * torch.rand(mask.shape, device="cuda:0", generator=gen)).argmax(1).to(torch.int32)
        host.send(ids, act.cpu().numpy())
        send_device_tensors(dev, act.contiguous(), torch.as_tensor(ids, device="cuda:0"))
    host.close()
    dev.close()


@pytest.mark.parametrize("name", ONE_EACH)
def test_fixture_envs_as_last_rows_of_a_big_pool(name):
    g = fixture(name)
    steps, m = g["actions"].shape
    steps = min(steps, 200)
    n = 65536
    seeds = np.arange(n, dtype=np.int64) * 7 + 11
    seeds[n - m:] = int(g["seed"]) + np.arange(m)
    pool = _pool(name, g, n=n, env_seed=[int(s) for s in seeds])
    ids = np.arange(n, dtype=np.int32)
    rng = np.random.default_rng(5)
    pool.reset(ids)
    rows = slice(n - m, n)
    prows = slice(2 * (n - m), 2 * n)
    for t in range(steps + 1):
        out = pool.recv_dict()
        check_rows({k: np.asarray(v)[prows if k in PER_PLAYER else rows] for k, v in out.items()}, g, t, name,
                   id_offset=n - m)
        if t < steps:
            act = rng.integers(-1, ACTIONS[game(name)] + 1, n).astype(np.int32)
            act[rows] = g["actions"][t]
            pool.send(ids, act)
    pool.close()


@pytest.mark.parametrize("name", ONE_EACH)
def test_sharded_pool_replays_fixture(name):
    """device=[0, 0]: two shards (env_id_offset 0 and n/2) replay the fixture's envs like one pool; the
    per-player keys of the two shards are joined per env."""
    g = fixture(name)
    steps, n = g["actions"].shape
    steps = min(steps, 200)
    env = envpool.make(task_id(name), "gymnasium", num_envs=n, device=[0, 0], **_kw(name, g))
    obs, info = env.reset()
    assert np.array_equal(info["env_id"], np.arange(n))
    assert np.array_equal(info["players"]["env_id"], np.repeat(np.arange(n), 2))
    for t in range(steps):
        obs, rew, term, trunc, info = env.step(g["actions"][t])
        assert np.array_equal(rew, g["reward"][t + 1].ravel()), (name, t)
        assert np.array_equal(term | trunc, g["done"][t + 1]), (name, t)
        assert np.array_equal(obs, g["obs"][t + 1].reshape(2 * n, *g["obs"].shape[3:])), (name, t)
    # a batch whose ids interleave the shards
    sub = np.array([n - 1, 0, n // 2, 1], np.int32)
    env.send(np.zeros(4, np.int32), sub)
    obs, rew, term, trunc, info = env.recv()
    assert np.array_equal(info["env_id"], sub)
    assert np.array_equal(info["players"]["env_id"], np.repeat(sub, 2))
    assert obs.shape == (8, *g["obs"].shape[3:])
    env.close()


def test_live_pool_multi_player_checks():
    env = envpool.make("Hex-v1", "gymnasium", num_envs=3)
    obs, info = env.reset()
    assert obs.shape == (6, 11, 11, 4)
    assert np.array_equal(info["players"]["env_id"], [0, 0, 1, 1, 2, 2])
    with pytest.raises(ValueError, match="players.env_id"):
        env.send({"action": np.zeros(3, np.int32), "players": {"env_id": np.array([2, 1, 0], np.int32)}})
    obs, rew, term, trunc, info = env.step(np.array([0, 60, 120], np.int32))
    assert rew.shape == (6,) and term.shape == (3,)
    env.close()


@pytest.mark.parametrize("name", ONE_EACH)
def test_set_state_round_trip(name):
    g = fixture(name)
    steps, n = g["actions"].shape
    ids = np.arange(n, dtype=np.int32)
    pool = _pool(name, g)
    pool.reset(ids)
    pool.recv_dict()
    for t in range(min(steps, 30)):
        pool.send(ids, g["actions"][t])
        pool.recv_dict()
    st = pool.get_state()
    other = st.copy()
    other[:, 2:] = st[::-1, 2:]
    pool.set_state(other)
    assert np.array_equal(pool.get_state()[:, 2:], other[:, 2:])
    pool.set_state(st)
    assert np.array_equal(pool.get_state(), st)
    pool.close()
