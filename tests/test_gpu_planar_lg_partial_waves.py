"""Bit-identity pin of the lane-group planar kernel (K3', mujoco_planar_lg.hip) where its waves are only partly filled
and episodes end: pools of 48 and 96 envs (lanes with no env at all, lanes that never touch anything and only ever
see the slot a lane reads once its own set has run out), HalfCheetah and Walker2d on groups of 2 and of 4 lanes and on 4
lanes at two waves per SIMD, max_episode_steps = 25 so that auto-resets fall inside the 120 seeded random-action steps.
Every state key of every step is hashed; the digests are compared with tests/golden/planar_lg_partial_digests.json.

The digests were generated with the build of the parent commit of the change that added this file (the kernel before
its active-set masks were encoded by visit index), so they pin what that kernel computed, not what this one does.
Each configuration runs in a child process of its own under a time limit.

Regenerate (only when the arithmetic is meant to change):  python tests/test_gpu_planar_lg_partial_waves.py --write
"""
import hashlib
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "planar_lg_partial_digests.json")
STEPS = 120
MAX_EPISODE_STEPS = 25
TIME_LIMIT_S = 120
# name -> (task, num_envs, planar_layout, planar_waves)
CONFIGS = {f"{task}-{n}-kl{kl}" + ("-w2" if w == 2 else ""): (task, n, kl, w)
           for task in ("HalfCheetah", "Walker2d") for n in (48, 96) for kl, w in ((2, 1), (4, 1), (4, 2))}


def _digests(task, n, layout, waves):
    """Runs in the child: per state key, sha256 over that key's bytes of every step."""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from envpool_amd.core.device_pool import DevicePool
    from envpool_amd.torch_interop import recv_device_tensors, send_device_tensors

    pool = DevicePool(task, n, seed=5, max_episode_steps=MAX_EPISODE_STEPS,
                      params={"planar_layout": layout, "planar_waves": waves})
    adim = int(np.prod(pool.action_shape))
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(17)
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
    task, n, layout, waves = CONFIGS[name]
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", task, str(n), str(layout), str(waves)],
                       cwd=ROOT, capture_output=True, text=True, timeout=TIME_LIMIT_S)
    assert r.returncode == 0, (name, r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONFIGS))
def test_planar_lg_partial_waves_digest(name):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    got = _run_child(name)
    assert sorted(got) == sorted(want), (name, sorted(got), sorted(want))
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, (name, "state keys whose bits changed", bad)


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        print(json.dumps(_digests(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))))
    elif sys.argv[1] == "--write":
        res = {}
        for name in CONFIGS:  # stops at the first failing configuration
            res[name] = _run_child(name)
        with open(GOLDEN, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
