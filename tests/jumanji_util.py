"""Shared helpers of the Jumanji tests: the fixtures (tests/golden/make_jumanji_golden.py), their ids and
configs, and the engine parameters of a fixture."""
import functools
import glob
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REGISTRY = json.load(open(os.path.join(GOLDEN, "jumanji_registry.json")))
SPECS = json.load(open(os.path.join(GOLDEN, "jumanji_spec.json")))
IDS = sorted(REGISTRY)
NAMES = sorted(os.path.basename(p)[len("jumanji_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "jumanji_*.npz")))
PREFIX = {tid: REGISTRY[tid]["spec_cls"][:-len("EnvSpec")] for tid in IDS}


@functools.lru_cache(maxsize=None)
def _load(name):
    with np.load(os.path.join(GOLDEN, f"jumanji_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def fixture(name):
    """The fixture's arrays (a fresh dict over cached arrays: do not modify them)."""
    return dict(_load(name))


def task_id(name):
    return name.split("__")[0]


def extra_config(name):
    """The config keys a fixture sets on top of its id's defaults, typed like the spec's defaults."""
    tid = task_id(name)
    raw = json.loads(str(fixture(name)["config"]))
    import envpool_amd

    spec = envpool_amd.make_spec(tid)
    defaults = dict(zip(spec._config_keys, type(spec)._default_config_values))
    out = {}
    for k, v in raw.items():
        d = defaults[k]
        out[k] = (v in ("1", "True", "true")) if isinstance(d, bool) else int(v) if isinstance(d, int) else v
    return out


def config(name):
    """The fixture's full config (spec defaults + registered kwargs + its own keys), as make_spec builds it."""
    import envpool_amd

    return envpool_amd.make_spec(task_id(name), **extra_config(name)).config._asdict()


def params(name):
    """The engine parameters of a fixture (DevicePool(<native family>, params=...))."""
    from envpool_amd.jumanji import FAMILIES

    fd = FAMILIES[PREFIX[task_id(name)]]
    return fd.native, {k: float(v) for k, v in fd.native_params(config(name)).items()}


def state_keys(name):
    """The fixture's env state keys (after the common keys), as stored in the .npz."""
    return [k for k, _ in SPECS[task_id(name)]["state_spec"][8:]]
