"""Shared helpers of the MiniGrid tests: the 30 fixture ids, their configs and fixtures
(tests/golden/make_minigrid_golden.py), and the engine parameters of an id; and the same for the option
cases, configs outside the registered ids (make_minigrid_golden.py --options)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REGISTRY = json.load(open(os.path.join(GOLDEN, "minigrid_registry.json")))
SPECS = json.load(open(os.path.join(GOLDEN, "minigrid_spec.json")))
IDS = sorted(REGISTRY)
# case -> {"kwargs": what make() takes on top of a registered id of that env_name, "spec": the reference's spec}
OPTION_TABLE = json.load(open(os.path.join(GOLDEN, "minigrid_option_cases.json")))
OPTION_CASES = sorted(OPTION_TABLE)
# the registered id an option case is made from: its own kwargs are all overridden by the case's or are defaults
OPTION_BASE_ID = {"empty": "MiniGrid-Empty-8x8-v0", "doorkey": "MiniGrid-DoorKey-8x8-v0",
                  "distshift": "MiniGrid-DistShift1-v0", "crossing": "MiniGrid-LavaCrossingS9N1-v0",
                  "lava_gap": "MiniGrid-LavaGapS5-v0", "dynamic_obstacles": "MiniGrid-Dynamic-Obstacles-8x8-v0"}
KEYS = ["obs:direction", "obs:image", "obs:mission", "info:agent_pos", "info:mission_id", "reward", "done",
        "trunc", "elapsed_step", "step_type", "discount", "info:env_id"]


def fixture(task_id):
    return np.load(os.path.join(GOLDEN, f"minigrid_{task_id}.npz"))


def config(task_id):
    """The id's full config (spec defaults + its registered kwargs), as make_spec builds it."""
    import envpool_amd

    return envpool_amd.make_spec(task_id).config._asdict()


def params(task_id):
    """The engine parameters of an id (MiniGrid family, DevicePool(params=...))."""
    from envpool_amd.minigrid import _native_params

    return {k: float(v) for k, v in _native_params(config(task_id)).items()}


def option_fixture(case):
    return np.load(os.path.join(GOLDEN, f"minigrid_opt__{case}.npz"))


def option_kwargs(case, pair=tuple):
    """(registered id, make kwargs) of an option case; the pair keys as `pair` (tuple or list)."""
    kw = {k: pair(v) if isinstance(v, list) else v for k, v in OPTION_TABLE[case]["kwargs"].items()}
    return OPTION_BASE_ID[kw.pop("env_name")], kw


def option_config(case, pair=tuple):
    import envpool_amd

    task_id, kw = option_kwargs(case, pair)
    return envpool_amd.make_spec(task_id, **kw).config._asdict()


def option_params(case, pair=tuple):
    from envpool_amd.minigrid import _native_params

    return {k: float(v) for k, v in _native_params(option_config(case, pair)).items()}
