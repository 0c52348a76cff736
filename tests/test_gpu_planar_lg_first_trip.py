"""Bit-identity pin of the lane-group planar kernel (K3', mujoco_planar_lg.hip) at the smallest pools that reach every
form of its solver's first Newton trip (code of its own in plg::Solve): a full wave plus a wave that holds one env
(lanes with no env run the first trip unmasked like every other lane), on groups of 2 and of 4 lanes and on the
Hopper's single lane, Euler (HalfCheetah: 5 forward passes per env-step) and RK4 (Walker2d, Hopper: 16).  8 seeded
random-action env-steps from the reset state; every state key of every step is hashed and the digests are compared
with tests/golden/planar_lg_first_trip_digests.json.

The digests were generated with the build of the parent commit of the change that added this file (one loop body
for every trip), so they pin what that kernel computed.  The pool has no key for the solver's iteration cap: the
caps of one and two trips are driven on the CPU, tests/test_planar_lg_first_trip_host.py.

Regenerate (only when the arithmetic is meant to change):  python tests/test_gpu_planar_lg_first_trip.py --write
"""
import hashlib
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "planar_lg_first_trip_digests.json")
STEPS = 8
# name -> (task, num_envs, planar_layout); 0 = the pool's own choice (the Hopper's group of one lane)
CONFIGS = {
    "HalfCheetah-33-kl2": ("HalfCheetah", 33, 2),
    "HalfCheetah-17-kl4": ("HalfCheetah", 17, 4),
    "Walker2d-33-kl2": ("Walker2d", 33, 2),
    "Walker2d-33-kl4": ("Walker2d", 33, 4),
    "Hopper-65": ("Hopper", 65, 0),
}


def _digests(task, n, layout):
    """per state key, sha256 over that key's bytes of every step"""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from envpool_amd.core.device_pool import DevicePool
    from envpool_amd.torch_interop import recv_device_tensors, send_device_tensors

    params = {"planar_layout": layout} if layout else {}
    pool = DevicePool(task, n, seed=7, max_episode_steps=1000, params=params)
    adim = int(np.prod(pool.action_shape))
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(23)
    hashes = {}

    def absorb(out):
        for k, v in out.items():
            hashes.setdefault(k, hashlib.sha256()).update(np.ascontiguousarray(v.cpu().numpy()).tobytes())

    send_device_tensors(pool, None)
    absorb(recv_device_tensors(pool))
    for _ in range(STEPS):
        act = torch.as_tensor(rng.uniform(-1.0, 1.0, (n, adim)), device=dev)
        send_device_tensors(pool, act)
        absorb(recv_device_tensors(pool))
    pool.synchronize()
    return {k: h.hexdigest() for k, h in sorted(hashes.items())}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONFIGS))
def test_planar_lg_first_trip_digest(name):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    got = _digests(*CONFIGS[name])
    assert sorted(got) == sorted(want), (name, sorted(got), sorted(want))
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, (name, "state keys whose bits changed", bad)


if __name__ == "__main__":
    if sys.argv[1] == "--write":
        res = {name: _digests(*cfg) for name, cfg in CONFIGS.items()}
        with open(GOLDEN, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
