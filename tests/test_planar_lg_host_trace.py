"""Bit-identity pin of the lane-group planar step on the CPU: the host instantiation of the kernel source
(tests/cpu_harness/planar_lg_host.cpp over envpool_amd/csrc/mj_planar_lg.hip.h) steps 64 envs for 40 env-steps --
HalfCheetah and Walker2d on groups of 2 and 4 lanes, the Hopper on one -- and per env and env-step the solver's
iteration count and a hash of the state (qpos, qvel, qacc_warmstart) are compared with tests/golden/planar_lg_host_trace.npz.

The trace was recorded with the sources of the parent commit of the change that added this file (the lane-group kernel
before its active-set masks were encoded by visit index), once as built for the product and once with the exact line
search from the second Newton trip on (-DEPA_LG_LS_EXACT_AFTER=1, the fallback the benchmark never reaches).  A change to
the bookkeeping of the solver -- the active-row masks, the per-lane slot sets, the iteration counter -- that alters which
trips an env runs shows up in `iters` and in the state without a GPU.  The states are the host's (x86-64, no FMA
contraction): this pins the control flow and the operation order of the source, the GPU digests pin the device build.

Start states and actions come from an integer hash, not from a library generator, so they are the same everywhere.

Regenerate (only when the arithmetic is meant to change):  python tests/test_planar_lg_host_trace.py --write
"""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "planar_lg_host_trace.npz")
HARNESS = os.path.join(ROOT, "tests", "cpu_harness")
CSRC = os.path.join(ROOT, "envpool_amd", "csrc")
N_ENVS, N_STEPS = 64, 40
# name -> (model of planar_lg_step, lanes per env, mj_steps per env-step, dofs, rootz of the reset pose)
CONFIGS = {
    "HalfCheetah-kl2": (0, 2, 5, 9, 0.0),
    "HalfCheetah-kl4": (0, 4, 5, 9, 0.0),
    "Walker2d-kl2": (1, 2, 4, 9, 1.25),
    "Walker2d-kl4": (1, 4, 4, 9, 1.25),
    "Hopper-kl1": (3, 1, 4, 6, 1.25),
}
BUILDS = {"product": ("libplanar_lg_host.so", []), "exact": ("libplanar_lg_host_exact.so", ["-DEPA_LG_LS_EXACT_AFTER=1"])}


def _unit(seed, shape):
    """doubles in [-1, 1) from splitmix64 of (seed, index): exact integer arithmetic, no generator state"""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(11)).astype(np.float64) * 2.0 ** -52 - 1.0).reshape(shape)


def _lib(build):
    name, flags = BUILDS[build]
    so, src = os.path.join(HARNESS, name), os.path.join(HARNESS, "planar_lg_host.cpp")
    newest = max(os.path.getmtime(f) for f in [src] + [os.path.join(CSRC, x) for x in
                                                      ("mj_planar_lg.hip.h", "mj_cheetah.hip.h", "mj_cheetah_model.h")])
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared"] + flags + [src, "-o", so], check=True)
    L = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    L.planar_lg_step.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, ctypes.c_int, vp, vp, vp, vp]
    return L


def _trace(L, name):
    """(iters int32 [steps][envs], hash uint64 [steps][envs]): the first 8 bytes of sha256(qpos | qvel | warm)"""
    model, kl, nsub, nd, z0 = CONFIGS[name]
    seed = 1 + sorted(CONFIGS).index(name)
    q = np.zeros((N_ENVS, 9))
    v = np.zeros((N_ENVS, 9))
    w = np.zeros((N_ENVS, 9))
    q[:, :nd] = 0.1 * _unit(100 + seed, (N_ENVS, nd))
    q[:, 1] += z0
    v[:, :nd] = 0.5 * _unit(200 + seed, (N_ENVS, nd))
    act = np.zeros((N_STEPS, N_ENVS, 6))
    act[:, :, :nd - 3] = 1.2 * _unit(300 + seed, (N_STEPS, N_ENVS, nd - 3))  # (beyond +-1: the kernel clamps)
    iters = np.zeros((N_STEPS, N_ENVS), np.int32)
    hashes = np.zeros((N_STEPS, N_ENVS), np.uint64)
    qo, vo, wo = np.zeros(9), np.zeros(9), np.zeros(9)
    it = ctypes.c_int(0)
    for t in range(N_STEPS):
        for e in range(N_ENVS):
            a = np.ascontiguousarray(act[t, e])
            rc = L.planar_lg_step(model, kl, q[e].ctypes.data, v[e].ctypes.data, w[e].ctypes.data, a.ctypes.data, nsub,
                                  qo.ctypes.data, vo.ctypes.data, wo.ctypes.data, ctypes.byref(it))
            assert rc == 0, (name, t, e, rc)  # lanes that replicate a value agree bit for bit
            q[e], v[e], w[e] = qo, vo, wo
            iters[t, e] = it.value
            hashes[t, e] = np.frombuffer(hashlib.sha256(qo.tobytes() + vo.tobytes() + wo.tobytes()).digest()[:8], np.uint64)[0]
    assert np.isfinite(q).all() and np.isfinite(v).all(), name
    return iters, hashes


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("name", list(CONFIGS))
def test_planar_lg_host_trace(name, build):
    want = np.load(GOLDEN)
    iters, hashes = _trace(_lib(build), name)
    wi, wh = want[f"{build}/{name}/iters"], want[f"{build}/{name}/hash"]
    assert wi.shape == iters.shape and wi.sum() > N_STEPS * N_ENVS  # the constraint solver did run
    bad = np.argwhere(iters != wi)
    assert bad.size == 0, (name, build, "first (env-step, env) whose iteration count changed", bad[0].tolist(),
                           int(iters[tuple(bad[0])]), int(wi[tuple(bad[0])]))
    bad = np.argwhere(hashes != wh)
    assert bad.size == 0, (name, build, "first (env-step, env) whose state bits changed", bad[0].tolist())


if __name__ == "__main__":
    if sys.argv[1] == "--write":
        res = {}
        for build in BUILDS:
            L = _lib(build)
            for name in CONFIGS:
                iters, hashes = _trace(L, name)
                res[f"{build}/{name}/iters"], res[f"{build}/{name}/hash"] = iters, hashes
                print(build, name, "iters: sum", int(iters.sum()), "max", int(iters.max()),
                      "hist", np.bincount(iters.ravel())[:12].tolist())
        np.savez_compressed(GOLDEN, **res)
