"""Bit-identity pin of the lane-group planar kernel (K3', mujoco_planar_lg.hip) for the pass over the constraint rows
whose first end-sphere visit WRITES most of the Hessian accumulators (plg::RowsPass<.., kPeel>, code of its own in
front of the slot loop, groups of two lanes; groups of four keep the one loop and are pinned next to them) where every
other visit adds to them: pools of 33 envs (a full wave plus a wave that holds one
env: its other lanes take every visit on the sentinel record) and of 64 (two full waves at 2 lanes per env, four at 4),
HalfCheetah (Euler) on groups of 2 and of 4 lanes and Walker2d (RK4).  20 seeded random-action env-steps from the reset
state of seed 0 -- contacts are made and broken, waves with and without a slot to visit -- every state key of every
step is hashed and the digests are compared with DIGESTS below.

DIGESTS was generated with the build of the parent commit of the change that added this file (every visit adds to
accumulators zeroed in front of the loop), so it pins what that kernel computed.  The crafted states -- no contact at
all, one lane in contact, signed zeros in the Jacobian -- are driven on the CPU, tests/test_planar_lg_row_peel_host.py.

Regenerate (only when the arithmetic is meant to change):  python tests/test_gpu_planar_lg_row_peel.py --print
"""
import hashlib
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 20
# name -> (task, num_envs, planar_layout)
CONFIGS = {
    "HalfCheetah-33-kl2": ("HalfCheetah", 33, 2),
    "HalfCheetah-33-kl4": ("HalfCheetah", 33, 4),
    "HalfCheetah-64-kl2": ("HalfCheetah", 64, 2),
    "HalfCheetah-64-kl4": ("HalfCheetah", 64, 4),
    "Walker2d-33-kl2": ("Walker2d", 33, 2),
}
# name -> sha256 over every state key (sorted; name, then that key's bytes of every step)
DIGESTS = {
    "HalfCheetah-33-kl2": "304d59a73b26a1a48e346d0732426676ba178d63128ab0795fafd2f35c1948f6",
    "HalfCheetah-33-kl4": "6fea7fdd3eed0a4f366a176cb6e54077ecbaf3811a10bfa40aebc2822c8ac4e0",
    "HalfCheetah-64-kl2": "f7162d932ef6ae29c4b5fe64ce787cb366482a50a855febd5ea0cf03a50f0819",
    "HalfCheetah-64-kl4": "7af40cb5caea215a253938c9731a05c06d3a7921edc9f510ee7cb96d7266ee30",
    "Walker2d-33-kl2": "5084f07ac99b813cba161d7d97d0f2f5602638000cfb41eba86e34e530dc2346",
}


def _digest(task, n, layout):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from envpool_amd.core.device_pool import DevicePool
    from envpool_amd.torch_interop import recv_device_tensors, send_device_tensors

    pool = DevicePool(task, n, seed=0, max_episode_steps=1000, params={"planar_layout": layout})
    adim = int(np.prod(pool.action_shape))
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
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
    total = hashlib.sha256()
    for k, h in sorted(hashes.items()):
        total.update(k.encode() + b"\0" + h.digest())
    return total.hexdigest()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONFIGS))
def test_planar_lg_row_peel_digest(name):
    assert _digest(*CONFIGS[name]) == DIGESTS[name], (name, "the bits of some state key changed")


if __name__ == "__main__":
    if sys.argv[1] == "--print":
        print(json.dumps({name: _digest(*cfg) for name, cfg in CONFIGS.items()}, indent=4))
