"""PGX board games, CPU side: the registry and the specs against what the reference itself reports
(tests/golden/pgx_registry.json, pgx_spec.json), the multi-player checks of the binding, the engine's description
of the per-player keys, and the env logic of the kernel (envpool_amd/csrc/pgx_env.hip.h) built for the host by g++
and replayed bit-exact against every reference fixture, hidden state included."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import envpool_amd as envpool
from pgx_util import CODE, GAME, IDS, KEYS, NAMES, PER_PLAYER, REGISTRY, SPECS, fixture, game, hidden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER_IDS = ["Go9x9-v1", "ChineseGo19x19-v1", "KuhnPoker-v1", "LeducHoldem-v1", "Play2048-v1", "AnimalShogi-v1",
             "Backgammon-v1", "Chess-v1", "GardnerChess-v1", "Shogi-v1", "SparrowMahjong-v1"]


def _plain(v):
    if isinstance(v, (tuple, list)):
        return [_plain(x) for x in v]
    if isinstance(v, (np.floating, float)):
        return float(np.float32(v))
    if isinstance(v, np.generic):
        return v.item()
    return v


def test_four_ids_registered_like_the_reference():
    from envpool_amd.registration import registry

    envpool.list_all_envs()
    assert IDS == sorted(["TicTacToe-v1", "ConnectFour-v1", "Hex-v1", "Othello-v1"])
    mine = {t for t in registry.specs if registry.specs[t][0] == "envpool_amd.pgx"}
    assert mine == set(IDS)
    for tid in IDS:
        ref = REGISTRY[tid]
        import_path, spec_cls, kwargs = registry.specs[tid]
        assert spec_cls == ref["spec_cls"]
        assert registry.envpools[tid]["dm"][1] == ref["dm_cls"]
        assert registry.envpools[tid]["gymnasium"][1] == ref["gymnasium_cls"]
        got = {k: _plain(v) for k, v in kwargs.items() if k != "base_path"}
        assert got == {"task": ref["task"], "max_num_players": ref["max_num_players"]}, tid
        assert envpool.make_spec(tid).config.max_num_players == 2


@pytest.mark.parametrize("tid", OTHER_IDS)
def test_other_pgx_ids_are_not_registered(tid):
    assert tid not in envpool.list_all_envs()


@pytest.mark.parametrize("tid", IDS)
def test_spec_matches_reference(tid):
    gold = SPECS[tid]
    spec = envpool.make_spec(tid)
    keys = list(spec._config_keys)
    defaults = list(type(spec)._default_config_values)
    ref_keys = [k for k, _ in gold["default_config"]]
    assert keys[:len(ref_keys)] == ref_keys
    assert [_plain(v) for v in defaults[:len(ref_keys)]] == [_plain(v) for _, v in gold["default_config"]]
    for names, specs, ref in ((spec._state_keys, spec._state_spec, gold["state_spec"]),
                              (spec._action_keys, spec._action_spec, gold["action_spec"])):
        assert list(names) == [k for k, _ in ref]
        for s, (k, r) in zip(specs, ref):
            assert np.dtype(s[0]) == np.dtype(r["dtype"]), k
            assert list(s[1]) == r["shape"], k
            assert _plain(list(s[2])) == _plain(r["bounds"]), k
            assert _plain([list(x) for x in s[3]]) == _plain(r["elementwise"]), k


@pytest.mark.parametrize("players", [1, 3])
@pytest.mark.parametrize("route", ["gymnasium", "dm"])
def test_max_num_players_other_than_two_raises(players, route):
    with pytest.raises(ValueError, match="max_num_players"):
        envpool.make("TicTacToe-v1", route, num_envs=2, max_num_players=players)


def test_single_player_families_still_refuse_more_players():
    with pytest.raises(ValueError, match="single-player"):
        envpool.make("CartPole-v1", "gymnasium", num_envs=2, max_num_players=2)


class _Recorder:
    def __init__(self):
        self.sent = []

    def send(self, env_id, action):
        self.sent.append((np.asarray(env_id), np.asarray(action)))


def test_send_with_players_env_id_other_than_env_id_raises():
    """One action row per env: a send that routes player rows elsewhere is refused (documented divergence)."""
    from envpool_amd.pgx import OthelloGymnasiumEnvPool

    native_pool = OthelloGymnasiumEnvPool.__mro__[1]  # _OthelloEnvPool
    pool = object.__new__(native_pool)
    pool._pool = _Recorder()
    ids = np.arange(3, dtype=np.int32)
    act = np.array([19, 26, 37], np.int32)
    pool._send([ids, ids.copy(), act])
    assert len(pool._pool.sent) == 1
    with pytest.raises(ValueError, match="players.env_id"):
        pool._send([ids, ids[::-1].copy(), act])
    with pytest.raises(ValueError, match="players.env_id"):
        pool._send([ids, np.repeat(ids, 2), act])
    assert len(pool._pool.sent) == 1


@pytest.mark.parametrize("tid", IDS)
def test_engine_describes_per_player_keys(tid):
    """The C ABI: P = 2, per-player keys with a leading 2 in their per-row shape; every other key as the spec
    says; single-player families unchanged."""
    from envpool_amd.core import native

    fam = GAME[tid]
    assert native.family_players(fam) == 2
    keys = native.describe(fam)
    players = native.describe_state_players(fam)
    assert [k for k, _, _ in keys] == KEYS
    for (name, dtype, shape), p, (_, ref) in zip(keys, players, SPECS[tid]["state_spec"]):
        assert np.dtype(dtype) == np.dtype(ref["dtype"]), name
        if name in PER_PLAYER:
            assert p == 2 and list(shape) == [2] + ref["shape"][1:], name
        else:
            assert p == 1 and list(shape) == ref["shape"], name
    assert [k for k, _, _ in native.describe(fam, which="action")] == ["env_id", "players.env_id", "action"]
    for single in ("CartPole", "Maze", "MiniGrid"):
        assert native.family_players(single) == 1
        assert set(native.describe_state_players(single)) == {1}
        assert dict((k, s) for k, _, s in native.describe(single))["reward"] == ()
    with pytest.raises(ValueError):
        native.family_players("NoSuchGame")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pgx") / "libpgxhost.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "cpu_harness", "pgx_host.cpp"), "-o", out], check=True)
    return ctypes.CDLL(out)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_replay(lib, name, g):
    acts = np.ascontiguousarray(g["actions"], np.int32)
    steps, n = acts.shape
    seeds = (int(g["seed"]) + np.arange(n)).astype(np.int32)
    outs = {k: np.zeros_like(g[k]) for k in KEYS}
    code = CODE[game(name)]
    hid = np.zeros((steps + 1, n, lib.pgx_hidden_words(code)), np.int32)
    ptrs = (ctypes.c_void_p * len(KEYS))(*[outs[k].ctypes.data for k in KEYS])
    rc = lib.pgx_replay(code, n, steps, _ptr(seeds), _ptr(acts), int(g["max_episode_steps"]), ptrs, _ptr(hid))
    assert rc == 0
    return outs, hid


@pytest.mark.parametrize("name", NAMES)
def test_host_harness_replays_fixture_bit_exact(harness, name):
    g = fixture(name)
    outs, hid = host_replay(harness, name, g)
    for k in KEYS:
        assert np.array_equal(outs[k], g[k]), (name, k)
    assert np.array_equal(hid, hidden(g)), name


def test_fixtures_cover_the_quirks():
    """What the fixtures pin: the first-row-only discount, 2 player rows per env, trunc in the __trunc runs, an
    Othello illegal pass and an illegal Hex swap among the actions."""
    for name in NAMES:
        g = fixture(name)
        d = g["discount"]
        assert (d[..., 1] == 0).all() and (d[..., 0] == ~g["done"]).all(), name
        assert (g["info:players.env_id"] == np.arange(g["actions"].shape[1])[None, :, None]).all(), name
        assert (g["info:players.id"] == [0, 1]).all(), name
        if name.endswith("__trunc"):
            assert g["trunc"].any(), name
    assert (fixture("Othello-v1")["actions"] == 64).any() and (fixture("Hex-v1")["actions"] == 121).any()
