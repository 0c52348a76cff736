"""Helpers for the `-m gpu` parity tests (call the product through the C ABI)."""
import importlib

import numpy as np

from envpool_amd.core.device_pool import DevicePool
from oracle_cases import CASES

PARAM_NAMES = {
    "Pendulum": ("version",),
    "FrozenLake": ("size",),
    "CliffWalking": ("is_slippery",),
    "Blackjack": ("natural", "sab"),
    "Catch": ("height", "width"),
}


def make_hip_pool(name, n, seed, extra_params=None, **kw):
    c = CASES[name]
    params = dict(zip(PARAM_NAMES.get(c["task"], ()), c["extra"]))
    params.update(extra_params or {})
    return DevicePool(c["task"], n, seed=seed, max_episode_steps=c["max_steps"],
                      params=params, **kw)


def registered_pool(task, n, seed, engine_keys=None, **make_kwargs):
    """The DevicePool that `envpool_amd.make(task, num_envs=n, seed=seed, **make_kwargs)` builds -- the family's own
    native_params of the id's config -- with `engine_keys` on top: engine keys ("mt_tile", "classic_block", ...) are
    no config keys and do not pass through `make`."""
    import envpool_amd
    from envpool_amd.registration import registry

    import_path, spec_cls, _ = registry.specs[task]
    mod = importlib.import_module(import_path)
    name = spec_cls[:-len("EnvSpec")]
    if import_path.endswith("mujoco.gym"):
        name = name[len("Gym"):]
    families = getattr(mod, "FAMILIES", None)
    fd = families[name] if families else getattr(mod, "_" + name)
    conf = envpool_amd.make_spec(task, num_envs=n, seed=seed, **make_kwargs).config._asdict()
    params = {k: float(v) for k, v in fd.native_params(conf).items()}
    params.update({k: float(v) for k, v in (engine_keys or {}).items()})
    return DevicePool(fd.native, n, batch_size=conf["batch_size"], seed=seed, env_seed=list(conf["env_seed"]) or None,
                      max_episode_steps=conf["max_episode_steps"], env_id_offset=conf["env_id_offset"], params=params)


class HipAsOracle:
    """DevicePool with the tiny reset()/step() -> dict surface of oracle.orc."""

    def __init__(self, pool):
        self.pool = pool
        self.ids = np.arange(pool.num_envs, dtype=np.int32)

    def reset(self, ids=None):
        self.pool.reset(self.ids if ids is None else ids)
        return self._flat(self.pool.recv_dict())

    def step(self, action, ids=None):
        self.pool.send(self.ids if ids is None else ids, action)
        return self._flat(self.pool.recv_dict())

    @staticmethod
    def _flat(d):
        return {k: v.reshape(v.shape[0], -1) for k, v in d.items()}
