"""Bit-identity pin of the lane-group planar kernel (K3', mujoco_planar_lg.hip): HalfCheetah, Walker2d and Hopper pools
of 65536 envs, and HalfCheetah at 8192 (the 4-lane layout), step 200 seeded random-action steps on the device path;
every state key of every step is hashed and the digests are compared with tests/golden/planar_lg_digests.json.

The digests were generated with the build of the parent commit of the change that added this file (the lane-group
kernel before its instruction-count pass), so any change to an env's fp64 operation sequence -- operands, order, FMA
contraction -- shows up here, not only a change large enough to cross the oracle tolerances of test_gpu_mujoco.py.
Each configuration runs in a child process of its own under a time limit.

Regenerate (only when the arithmetic is meant to change):  python tests/test_gpu_planar_lg_digest.py --write
"""
import hashlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "planar_lg_digests.json")
STEPS = 200
TIME_LIMIT_S = 300
# name -> (task, num_envs, planar_layout); 0 = the pool's own choice (2 lanes per env at 65536, the Hopper's one)
CONFIGS = {
    "HalfCheetah-65536": ("HalfCheetah", 65536, 0),
    "Walker2d-65536": ("Walker2d", 65536, 0),
    "Hopper-65536": ("Hopper", 65536, 0),
    "HalfCheetah-8192-kl4": ("HalfCheetah", 8192, 4),
}


def _digests(task, n, layout):
    """Runs in the child: per state key, sha256 over that key's bytes of every step."""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from envpool_amd.core.device_pool import DevicePool
    from envpool_amd.torch_interop import recv_device_tensors, send_device_tensors

    params = {"planar_layout": layout} if layout else {}
    pool = DevicePool(task, n, seed=3, max_episode_steps=1000, params=params)
    adim = int(np.prod(pool.action_shape))
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
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


def _run_child(name):
    task, n, layout = CONFIGS[name]
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", task, str(n), str(layout)],
                       cwd=ROOT, capture_output=True, text=True, timeout=TIME_LIMIT_S)
    assert r.returncode == 0, (name, r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONFIGS))
def test_planar_lg_digest(name):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    got = _run_child(name)
    assert sorted(got) == sorted(want), (name, sorted(got), sorted(want))
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, (name, "state keys whose bits changed", bad)


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        print(json.dumps(_digests(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))))
    elif sys.argv[1] == "--write":
        res = {}
        for name in CONFIGS:  # stops at the first failing configuration
            res[name] = _run_child(name)
        with open(GOLDEN, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
