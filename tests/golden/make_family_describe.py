"""Records what the C ABI says about every env family and every registered (non-Atari) task id into
tests/golden/family_describe.json, which tests/test_family_describe.py compares the library with:

    python tests/golden/make_family_describe.py

Per family index i: epa_family_name(i), epa_family_players, and epa_describe_state (name, dtype, row shape),
epa_describe_state_players and epa_describe_action with no params.  Per task id: the same three describe calls with
the native params its FamilyDef derives from the id's default config.  Needs only the built library, no GPU.
"""
import importlib
import inspect
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import envpool_amd as envpool  # noqa: E402
from envpool_amd.core import native  # noqa: E402
from envpool_amd.registration import registry  # noqa: E402


def keys(family, params, which):
    return [[name, np.dtype(dtype).str, list(shape)] for name, dtype, shape in native.describe(family, params, which)]


def describe(family, params=None):
    return {"state": keys(family, params, "state"),
            "state_players": native.describe_state_players(family, params),
            "action": keys(family, params, "action")}


def task_params(task_id):
    """(native family, native params) of a registered id, or None for a family with its own pool factory (Atari)."""
    import_path, spec_cls, _ = registry.specs[task_id]
    fd = inspect.getclosurevars(getattr(importlib.import_module(import_path), spec_cls).__init__).nonlocals["fd"]
    if fd.pool_factory is not None:
        return None
    conf = envpool.make_spec(task_id)._conf
    return fd.native, {k: float(v) for k, v in fd.native_params(conf).items()}


def collect():
    families = []
    for i in range(native.lib().epa_num_families()):
        name = native.lib().epa_family_name(i).decode()
        families.append({"name": name, "players": native.family_players(name), **describe(name)})
    tasks = {}
    for task_id in envpool.list_all_envs():
        tp = task_params(task_id)
        if tp is not None:
            tasks[task_id] = {"family": tp[0], "params": tp[1], **describe(*tp)}
    return {"families": families, "tasks": tasks}


if __name__ == "__main__":
    out = os.path.join(HERE, "family_describe.json")
    with open(out, "w") as f:
        json.dump(collect(), f, indent=1)
        f.write("\n")
    print(f"wrote {out}")
