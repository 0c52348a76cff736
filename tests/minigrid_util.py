"""Shared helpers of the MiniGrid tests: the 30 fixture ids, their configs and fixtures
(tests/golden/make_minigrid_golden.py), and the engine parameters of an id."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REGISTRY = json.load(open(os.path.join(GOLDEN, "minigrid_registry.json")))
SPECS = json.load(open(os.path.join(GOLDEN, "minigrid_spec.json")))
IDS = sorted(REGISTRY)
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
