"""MiniGrid navigation family, CPU side: the spec and the registry against what the reference itself
reports (tests/golden/minigrid_spec.json, minigrid_registry.json), and the env logic of the kernel
(envpool_amd/csrc/minigrid_env.hip.h) built for the host by g++ and replayed against every reference
fixture, grids included; the same for the option cases (configs outside the registered ids,
tests/golden/minigrid_option_cases.json), plus the route of their kwargs into the engine parameters."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import envpool_amd as envpool
from minigrid_util import (IDS, OPTION_CASES, OPTION_TABLE, REGISTRY, SPECS, config, fixture, option_config,
                           option_fixture, option_kwargs, option_params)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain(v):
    if isinstance(v, (tuple, list)):
        return [_plain(x) for x in v]
    if isinstance(v, (np.floating, float)):
        return float(np.float32(v))
    if isinstance(v, np.generic):
        return v.item()
    return v


def test_thirty_ids_registered_like_the_reference():
    from envpool_amd.registration import registry

    envpool.list_all_envs()
    assert len(IDS) == 30
    mine = {t for t in registry.specs if registry.specs[t][0] == "envpool_amd.minigrid"}
    assert mine == set(IDS)
    for tid in IDS:
        import_path, spec_cls, kwargs = registry.specs[tid]
        assert spec_cls == "MiniGridEnvSpec"
        assert registry.envpools[tid]["dm"][1] == "MiniGridDMEnvPool"
        assert registry.envpools[tid]["gymnasium"][1] == "MiniGridGymnasiumEnvPool"
        got = {k: _plain(v) for k, v in kwargs.items() if k != "base_path"}
        assert got == REGISTRY[tid], tid


@pytest.mark.parametrize("task_id", ["BabyAI-GoToLocal-v0", "MiniGrid-Unlock-v0", "MiniGrid-KeyCorridorS3R1-v0",
                                     "MiniGrid-MultiRoom-N2-S4-v0", "MiniGrid-Fetch-5x5-N2-v0"])
def test_out_of_scope_ids_are_not_registered(task_id):
    assert task_id not in envpool.list_all_envs()
    with pytest.raises(AssertionError):
        envpool.make(task_id, "gymnasium", num_envs=1)


def _assert_spec_matches(spec, gold):
    keys = list(spec._config_keys)
    defaults = list(type(spec)._default_config_values) if hasattr(type(spec), "_default_config_values") else None
    ref_keys = [k for k, _ in gold["default_config"]]
    assert keys[:len(ref_keys)] == ref_keys
    if defaults is not None:
        assert [_plain(v) for v in defaults[:len(ref_keys)]] == [_plain(v) for _, v in gold["default_config"]]
    for names, specs, ref in ((spec._state_keys, spec._state_spec, gold["state_spec"]),
                              (spec._action_keys, spec._action_spec, gold["action_spec"])):
        assert list(names) == [k for k, _ in ref]
        for s, (k, r) in zip(specs, ref):
            assert np.dtype(s[0]) == np.dtype(r["dtype"]), k
            assert list(s[1]) == r["shape"], k
            assert _plain(list(s[2])) == _plain(r["bounds"]), k


@pytest.mark.parametrize("task_id", IDS)
def test_spec_matches_reference(task_id):
    _assert_spec_matches(envpool.make_spec(task_id), SPECS[task_id])


@pytest.mark.parametrize("case", OPTION_CASES)
def test_option_spec_matches_reference(case):
    """make_spec(<a registered id of the env_name>, **kwargs) against the reference's spec of that config."""
    task_id, kw = option_kwargs(case)
    spec = envpool.make_spec(task_id, **kw)
    _assert_spec_matches(spec, OPTION_TABLE[case]["spec"])
    # the config is the reference's defaults plus the case's kwargs: the registered id adds nothing of its own
    conf = spec.config._asdict()
    from envpool_amd.core.binding import COMMON_CONFIG

    common = {k for k, _ in COMMON_CONFIG}
    want = dict((k, v) for k, v in OPTION_TABLE[case]["spec"]["default_config"] if k not in common)
    want.update(OPTION_TABLE[case]["kwargs"])
    assert {k: _plain(conf[k]) for k in want} == {k: _plain(v) for k, v in want.items()}
    by_key = dict(zip(spec._state_keys, spec._state_spec))
    assert tuple(by_key["info:agent_pos"][2]) == (0, max(conf["size"], conf["width"], conf["height"], 25))
    assert tuple(dict(zip(spec._action_keys, spec._action_spec))["action"][2]) == (0, conf["action_max"])


def test_unsupported_config_raises():
    with pytest.raises(ValueError):
        envpool.make_spec("MiniGrid-Empty-5x5-v0", env_name="wfc")
    with pytest.raises(ValueError):
        envpool.make_spec("MiniGrid-Empty-5x5-v0", agent_view_size=5)


def test_decode_mission():
    from envpool_amd.minigrid import MiniGridGymnasiumEnvPool, decode_mission

    row = np.zeros(96, np.uint8)
    row[:14] = np.frombuffer(b"reach the goal", np.uint8)
    assert decode_mission(row) == "reach the goal"
    two = np.stack([row, np.zeros(96, np.uint8)])
    assert list(decode_mission(two)) == ["reach the goal", ""]
    full = np.full(96, ord("a"), np.uint8)
    assert decode_mission(full) == "a" * 96
    assert MiniGridGymnasiumEnvPool.decode_mission(row) == "reach the goal"
    # the fixtures' missions are the reference's texts
    assert decode_mission(fixture("MiniGrid-DoorKey-5x5-v0")["obs__mission"][0, 0]) == \
        "use the key to open the door and then get to the goal"


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mg") / "libmghost.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "cpu_harness", "minigrid_host.cpp"), "-o", out], check=True)
    return ctypes.CDLL(out)


def task_cfg(conf: dict, max_tries: int = 1 << 20) -> np.ndarray:
    """mg::TaskCfg of a config, as csrc/minigrid.hip's MakeTaskCfg derives it."""
    from envpool_amd.minigrid import ENV_NAMES

    task = ENV_NAMES[conf["env_name"]]
    w = h = conf["size"]
    if conf["env_name"] == "distshift":
        w, h = conf["width"], conf["height"]
    if conf["env_name"] == "four_rooms":
        w = h = 19
    n_obst = 0
    if conf["env_name"] == "dynamic_obstacles":
        n = conf["n_obstacles"]
        n_obst = n if n <= conf["size"] // 2 + 1 else conf["size"] // 2
    obstacle = (2 | (5 << 4)) if conf["obstacle_type"] == "wall" else 9
    see = int(conf["env_name"] in ("empty", "distshift", "dynamic_obstacles"))
    sx, sy = conf["agent_start_pos"]
    return np.array([task, w, h, conf["size"], sx, sy, conf["agent_start_dir"], conf["num_crossings"], obstacle,
                     conf["strip2_row"], n_obst, conf["max_episode_steps"], max_tries, see], np.int32)


def params_task_cfg(p: dict, max_episode_steps: int, max_tries: int = 1 << 20) -> np.ndarray:
    """mg::TaskCfg of the engine parameters `_native_params` gives: the keys csrc/minigrid.hip's MakeTaskCfg reads."""
    task = int(p["env_name_code"])
    size = int(p["size"])
    w, h = (int(p["width"]), int(p["height"])) if task == 2 else (19, 19) if task == 6 else (size, size)
    n = int(p["n_obstacles"])
    n_obst = (n if n <= size // 2 + 1 else size // 2) if task == 5 else 0
    return np.array([task, w, h, size, p["start_x"], p["start_y"], p["start_dir"], p["num_crossings"],
                     (2 | (5 << 4)) if p["obstacle_wall"] else 9, p["strip2_row"], n_obst, max_episode_steps, max_tries,
                     int(task in (0, 2, 5))], np.int32)


@pytest.mark.parametrize("case", OPTION_CASES)
def test_option_engine_params_give_the_task_cfg(case):
    """The kwargs' route into the engine (make_spec -> _native_params) and the host harness (task_cfg) agree."""
    conf = option_config(case)
    got = params_task_cfg(option_params(case), conf["max_episode_steps"])
    np.testing.assert_array_equal(got, task_cfg(conf))
    g = option_fixture(case)
    assert (got[1], got[2]) == (int(g["width"]), int(g["height"]))
    assert got[11] == OPTION_TABLE[case]["kwargs"]["max_episode_steps"]


@pytest.mark.parametrize("case", [c for c in OPTION_CASES if "agent_start_pos" in OPTION_TABLE[c]["kwargs"]])
def test_option_pair_key_as_tuple_and_list(case):
    want = tuple(OPTION_TABLE[case]["kwargs"]["agent_start_pos"])
    for pair in (tuple, list):
        conf = option_config(case, pair)
        assert tuple(conf["agent_start_pos"]) == want
        p = option_params(case, pair)
        assert (p["start_x"], p["start_y"]) == want
    assert option_params(case, tuple) == option_params(case, list)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_replay(lib, conf, g, max_tries=1 << 20):
    acts = np.ascontiguousarray(g["actions"], np.int32)
    steps, n = acts.shape
    w, h = int(g["width"]), int(g["height"])
    seeds = (int(g["seed"]) + np.arange(n)).astype(np.int32)
    out = dict(dir=np.zeros((steps + 1, n), np.int32), image=np.zeros((steps + 1, n, 7, 7, 3), np.uint8),
               pos=np.zeros((steps + 1, n, 2), np.int32), reward=np.zeros((steps + 1, n), np.float32),
               done=np.zeros((steps + 1, n), np.uint8), trunc=np.zeros((steps + 1, n), np.uint8),
               elapsed=np.zeros((steps + 1, n), np.int32), grid=np.zeros((steps + 1, n, w * h * 3), np.uint8))
    rc = lib.mg_replay(_ptr(task_cfg(conf, max_tries)), n, steps, _ptr(seeds), _ptr(acts), _ptr(out["dir"]),
                       _ptr(out["image"]), _ptr(out["pos"]), _ptr(out["reward"]), _ptr(out["done"]),
                       _ptr(out["trunc"]), _ptr(out["elapsed"]), _ptr(out["grid"]))
    return rc, out


@pytest.mark.parametrize("task_id", IDS + [f"opt__{c}" for c in OPTION_CASES])
def test_host_build_replays_reference_fixture(harness, task_id):
    if task_id.startswith("opt__"):
        g, conf = option_fixture(task_id[5:]), option_config(task_id[5:])
    else:
        g, conf = fixture(task_id), config(task_id)
    rc, o = host_replay(harness, conf, g)
    assert rc == 0
    np.testing.assert_array_equal(o["dir"], g["obs__direction"])
    np.testing.assert_array_equal(o["pos"], g["info__agent_pos"])
    np.testing.assert_array_equal(o["elapsed"], g["elapsed_step"])
    np.testing.assert_array_equal(o["reward"], g["reward"])
    np.testing.assert_array_equal(o["done"].astype(bool), g["done"])
    np.testing.assert_array_equal(o["trunc"].astype(bool), g["trunc"])
    np.testing.assert_array_equal(o["grid"], g["grid"])
    np.testing.assert_array_equal(o["image"], g["obs__image"])


def test_host_build_bounds_rejection_sampling(harness):
    """minigrid_max_tries = 1 on FourRooms: some first resets run out of tries instead of spinning."""
    g = fixture("MiniGrid-FourRooms-v0")
    conf = config("MiniGrid-FourRooms-v0")
    fails = 0
    for seed in range(64):
        g2 = dict(g)
        g2["seed"] = np.int32(seed * 8)
        rc, _ = host_replay(harness, conf, g2, max_tries=1)
        fails += rc != 0
    assert 0 < fails < 64
