"""Jumanji board puzzles, CPU side: the registry and the specs against what the reference itself reports
(tests/golden/jumanji_registry.json, jumanji_spec.json), the host parsing of the initial-state keys, the
rejected replay hooks, and the env logic of the kernel (envpool_amd/csrc/jumanji_env.hip.h) built for the
host by g++ and replayed bit-exact against every reference fixture, hidden state included."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import envpool_amd as envpool
from jumanji_util import IDS, NAMES, PREFIX, REGISTRY, SPECS, config, fixture, state_keys, task_id

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OTHER_IDS = ["BinPack-v2", "CVRP-v1", "Cleaner-v0", "Connector-v2", "FlatPack-v0", "GraphColoring-v1", "JobShop-v0",
             "Knapsack-v1", "LevelBasedForaging-v0", "MMST-v0", "MultiCVRP-v0", "PacMan-v1", "RobotWarehouse-v0",
             "SearchAndRescue-v0", "Sokoban-v0", "Sudoku-v0", "Sudoku-very-easy-v0", "TSP-v1", "Tetris-v0"]


def _plain(v):
    if isinstance(v, (tuple, list)):
        return [_plain(x) for x in v]
    if isinstance(v, (np.floating, float)):
        return float(np.float32(v))
    if isinstance(v, np.generic):
        return v.item()
    return v


def test_seven_ids_registered_like_the_reference():
    from envpool_amd.registration import registry

    envpool.list_all_envs()
    assert IDS == sorted(["Game2048-v1", "Minesweeper-v0", "SlidingTilePuzzle-v0", "RubiksCube-v0",
                          "RubiksCube-partly-scrambled-v0", "Snake-v1", "Maze-v0"])
    mine = {t for t in registry.specs if registry.specs[t][0] == "envpool_amd.jumanji"}
    assert mine == set(IDS) | {f"Jumanji/{t}" for t in IDS}
    for tid in IDS:
        ref = REGISTRY[tid]
        assert ref["aliases"] == [f"Jumanji/{tid}"]
        for name in (tid, *ref["aliases"]):
            import_path, spec_cls, kwargs = registry.specs[name]
            assert spec_cls == ref["spec_cls"]
            assert registry.envpools[name]["dm"][1] == ref["dm_cls"]
            assert registry.envpools[name]["gymnasium"][1] == ref["gymnasium_cls"]
            got = {k: _plain(v) for k, v in kwargs.items() if k != "base_path"}
            assert got == {"max_episode_steps": ref["max_episode_steps"]}, name
        assert envpool.make_spec(tid).config.max_episode_steps == ref["max_episode_steps"]


@pytest.mark.parametrize("tid", OTHER_IDS)
def test_other_jumanji_ids_are_not_registered(tid):
    envs = envpool.list_all_envs()
    assert tid not in envs and f"Jumanji/{tid}" not in envs
    with pytest.raises(AssertionError):
        envpool.make(tid, "gymnasium", num_envs=1)


@pytest.mark.parametrize("tid", IDS)
def test_spec_matches_reference(tid):
    gold = SPECS[tid]
    for name in (tid, f"Jumanji/{tid}"):
        spec = envpool.make_spec(name)
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


@pytest.mark.parametrize("key,value", [("game2048_replay_boards", "0,1")])
def test_game2048_replay_hook_raises(key, value):
    with pytest.raises(ValueError):
        envpool.make_spec("Game2048-v1", **{key: value})
    with pytest.raises(ValueError):
        envpool.make("Jumanji/Game2048-v1", "gymnasium", num_envs=1, **{key: value})


@pytest.mark.parametrize("key", ["minesweeper_replay_boards", "minesweeper_replay_rewards", "minesweeper_replay_done"])
def test_minesweeper_replay_hooks_raise(key):
    with pytest.raises(ValueError):
        envpool.make_spec("Minesweeper-v0", **{key: "1"})
    with pytest.raises(ValueError):
        envpool.make("Minesweeper-v0", "dm", num_envs=1, **{key: "1"})


def test_host_parsing_of_initial_state_keys():
    from envpool_amd.jumanji import engine_config

    spec = lambda tid, **kw: envpool.make_spec(tid, **kw).config._asdict()  # noqa: E731
    # Minesweeper: out-of-range locations dropped, duplicates merged; none left = the random default
    cfg, init = engine_config("Minesweeper", spec("Minesweeper-v0", minesweeper_mine_locations="5,3,5,100,-1"))
    assert cfg[2] == 1 and cfg[5] == 2 and np.flatnonzero(init).tolist() == [3, 5]
    cfg, init = engine_config("Minesweeper", spec("Minesweeper-v0", minesweeper_mine_locations="100"))
    assert cfg[2] == 0 and cfg[5] == 10 and not any(init)
    # positions: clamped, the default without ',', the text after the first ',' read by stoi
    cfg, _ = engine_config("Maze", spec("Maze-v0", maze_agent_position="-3,14", maze_target_position="7"))
    assert cfg[6:10] == [0, 9, 9, 9]
    cfg, _ = engine_config("Snake", spec("Snake-v1", snake_head_position=" 4,5,6"))
    assert cfg[2] == 1 and cfg[6:10] == [4, 5, 0, 1]
    # boards: a short list keeps the default tail, a trailing ',' is no token, stoi ignores trailing text
    cfg, init = engine_config("SlidingTilePuzzle", spec("SlidingTilePuzzle-v0", sliding_tile_initial_puzzle="2,1x,"))
    assert init[:4] == [2, 1, 3, 4] and init[24] == 0
    cfg, init = engine_config("RubiksCube", spec("RubiksCube-v0", rubiks_cube_initial_cube="300,-1"))
    assert init[:3] == [44, -1, 0]  # static_cast<std::int8_t>
    with pytest.raises(ValueError):
        engine_config("Game2048", spec("Game2048-v1", game2048_initial_board="1,,2"))
    # RubiksCube-partly-scrambled: its own limit and scramble count
    cfg, _ = engine_config("RubiksCubePartlyScrambled", spec("RubiksCube-partly-scrambled-v0"))
    assert cfg[1] == 20 and cfg[4] == 20


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("jm") / "libjmhost.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "cpu_harness", "jumanji_host.cpp"), "-o", out], check=True)
    return ctypes.CDLL(out)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_replay(lib, name, g, max_tries=1 << 20, seed=None):
    from envpool_amd.jumanji import engine_config

    tid = task_id(name)
    conf = config(name)
    cfg, init = engine_config(PREFIX[tid], conf)
    cfg = np.array(cfg + [max_tries], np.int32)
    assert len(cfg) == lib.jm_cfg_words()
    init = np.array(init, np.int32)
    acts = np.ascontiguousarray(g["actions"], np.int32)
    steps, n = acts.shape[:2]
    act_dim = 1 if acts.ndim == 2 else acts.shape[2]
    seeds = ((int(g["seed"]) if seed is None else seed) + np.arange(n)).astype(np.int32)
    keys = state_keys(name)
    outs = [np.zeros_like(g[k.replace(":", "__")]) for k in keys]
    rows = np.array([o[0, 0].nbytes for o in outs], np.int32)
    ptrs = (ctypes.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
    limit = cfg[1] + 1 if cfg[1] > 0 else conf["max_episode_steps"]
    res = dict(reward=np.zeros((steps + 1, n), np.float32), done=np.zeros((steps + 1, n), np.uint8),
               trunc=np.zeros((steps + 1, n), np.uint8), elapsed_step=np.zeros((steps + 1, n), np.int32),
               hidden=np.zeros((steps + 1, n, g["hidden"].shape[2]), np.int32))
    rc = lib.jm_replay(_ptr(cfg), _ptr(init), n, steps, _ptr(seeds), _ptr(acts), act_dim, int(limit), ptrs,
                       _ptr(rows), len(outs), _ptr(res["reward"]), _ptr(res["done"]), _ptr(res["trunc"]),
                       _ptr(res["elapsed_step"]), _ptr(res["hidden"]))
    res.update({k.replace(":", "__"): o for k, o in zip(keys, outs)})
    return rc, res


@pytest.mark.parametrize("name", NAMES)
def test_host_build_replays_reference_fixture(harness, name):
    g = fixture(name)
    rc, o = host_replay(harness, name, g)
    assert rc == 0
    for k in ["reward", "elapsed_step", "hidden"] + [k.replace(":", "__") for k in state_keys(name)]:
        np.testing.assert_array_equal(o[k], g[k], err_msg=f"{name} {k}")
    np.testing.assert_array_equal(o["done"].astype(bool), g["done"], err_msg=name)
    np.testing.assert_array_equal(o["trunc"].astype(bool), g["trunc"], err_msg=name)


def test_host_build_bounds_snake_fruit_placement(harness):
    """snake_max_tries = 1: about 1 in 144 first fruit draws lands on the head; such resets fail instead of
    spinning, the default bound resets the same seeds."""
    g = fixture("Snake-v1")
    fails = 0
    for seed in range(0, 8 * 400, 8):
        rc, _ = host_replay(harness, "Snake-v1", {**g, "actions": g["actions"][:1]}, max_tries=1, seed=seed)
        fails += rc != 0
        if rc != 0:
            assert host_replay(harness, "Snake-v1", {**g, "actions": g["actions"][:1]}, seed=seed)[0] == 0
    assert 0 < fails < 400
