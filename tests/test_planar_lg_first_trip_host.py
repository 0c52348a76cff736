"""Bit-identity pin, on the CPU, of the first Newton trip of a forward pass of the lane-group planar step (plg::Solve),
which is code of its own: the host instantiation of the kernel source (tests/cpu_harness/planar_lg_first_trip_host.cpp
over planar_lg_host.cpp and envpool_amd/csrc/mj_planar_lg.hip.h) runs single forward passes with the solver's
iteration cap set by the test --

  cap1    max_iter = 1: only the first trip runs, then the gradient refresh behind the loop for the envs still live
  cap2    max_iter = 2: the first trip and one general trip
  full    max_iter = 50: the product's cap
  again   two passes at the same state, the second warm-started at the first one's result: the env is at its
          minimiser already and stops at the first test of the first trip (zero trips)

-- for HalfCheetah and Walker2d on groups of 2 and 4 lanes and the Hopper on one, at the start states, and after 2
and 5 env-steps of random actions (contacts made and broken).  Per lane the trips counted, qacc, M qacc and the
gradient are compared for exact equality with tests/golden/planar_lg_first_trip_host.npz, and so are the hashes of
the states the env-steps in between produce.

The golden file was recorded with the sources of the parent commit of the change that added this file (one loop body
for every trip).  The values are the host's (x86-64, no FMA contraction): this pins the control flow and the operation
order of the source; tests/test_gpu_planar_lg_first_trip.py pins the device build.

Regenerate (only when the arithmetic is meant to change):  python tests/test_planar_lg_first_trip_host.py --write
"""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "planar_lg_first_trip_host.npz")
HARNESS = os.path.join(ROOT, "tests", "cpu_harness")
CSRC = os.path.join(ROOT, "envpool_amd", "csrc")
N_ENVS = 8
AT_STEPS = (0, 2, 5)  # forward passes are taken at the states before these env-steps
KLV = 6  # values per lane: three torso dofs, three of the lane's leg
# name -> (model of planar_lg_step, lanes per env, mj_steps per env-step, dofs, rootz of the reset pose)
CONFIGS = {
    "HalfCheetah-kl2": (0, 2, 5, 9, 0.0),
    "HalfCheetah-kl4": (0, 4, 5, 9, 0.0),
    "Walker2d-kl2": (1, 2, 4, 9, 1.25),
    "Walker2d-kl4": (1, 4, 4, 9, 1.25),
    "Hopper-kl1": (3, 1, 4, 6, 1.25),
}
# name -> (max_iter, passes)
CASES = {"cap1": (1, 1), "cap2": (2, 1), "full": (50, 1), "again": (50, 2)}


def _unit(seed, shape):
    """doubles in [-1, 1) from splitmix64 of (seed, index): exact integer arithmetic, no generator state"""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(11)).astype(np.float64) * 2.0 ** -52 - 1.0).reshape(shape)


def _lib():
    so, src = os.path.join(HARNESS, "libplanar_lg_first_trip_host.so"), os.path.join(HARNESS, "planar_lg_first_trip_host.cpp")
    deps = [src, os.path.join(HARNESS, "planar_lg_host.cpp")] + [os.path.join(CSRC, x) for x in
                                                                ("mj_planar_lg.hip.h", "mj_cheetah.hip.h", "mj_cheetah_model.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", src, "-o", so], check=True)
    L = ctypes.CDLL(so)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.planar_lg_step.argtypes = [ci, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp]
    L.planar_lg_forward.argtypes = [ci, ci, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp]
    L.planar_lg_forward.restype = None
    return L


@pytest.fixture(scope="module")
def lib():
    return _lib()


def _run(L, name):
    """{key: array}: per case iters [state][env][lane] and qacc / ma / grad [state][env][KLV][lane]; hash [step][env]"""
    model, kl, nsub, nd, z0 = CONFIGS[name]
    seed = 11 + sorted(CONFIGS).index(name)
    n_steps = max(AT_STEPS)
    q = np.zeros((N_ENVS, 9))
    v = np.zeros((N_ENVS, 9))
    w = np.zeros((N_ENVS, 9))
    q[:, :nd] = 0.1 * _unit(100 + seed, (N_ENVS, nd))
    q[:, 1] += z0
    v[:, :nd] = 0.5 * _unit(200 + seed, (N_ENVS, nd))
    act = np.zeros((n_steps + 1, N_ENVS, 6))
    act[:, :, :nd - 3] = 1.2 * _unit(300 + seed, (n_steps + 1, N_ENVS, nd - 3))  # (beyond +-1: the kernel clamps)
    res = {f"{c}/iters": np.zeros((len(AT_STEPS), N_ENVS, kl), np.int32) for c in CASES}
    for c in CASES:
        for k in ("qacc", "ma", "grad"):
            res[f"{c}/{k}"] = np.zeros((len(AT_STEPS), N_ENVS, KLV, kl))
    res["hash"] = np.zeros((n_steps, N_ENVS), np.uint64)
    qo, vo, wo = np.zeros(9), np.zeros(9), np.zeros(9)
    it = ctypes.c_int(0)
    its = np.zeros(kl, np.int32)
    for t in range(n_steps + 1):
        for e in range(N_ENVS):
            a = np.ascontiguousarray(act[t, e])
            if t in AT_STEPS:
                s = AT_STEPS.index(t)
                for c, (max_iter, passes) in CASES.items():
                    out = [res[f"{c}/{k}"][s, e] for k in ("qacc", "ma", "grad")]
                    L.planar_lg_forward(model, kl, q[e].ctypes.data, v[e].ctypes.data, w[e].ctypes.data, a.ctypes.data,
                                        max_iter, passes, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data,
                                        its.ctypes.data)
                    res[f"{c}/iters"][s, e] = its
            if t == n_steps:
                continue
            rc = L.planar_lg_step(model, kl, q[e].ctypes.data, v[e].ctypes.data, w[e].ctypes.data, a.ctypes.data, nsub,
                                  qo.ctypes.data, vo.ctypes.data, wo.ctypes.data, ctypes.byref(it))
            assert rc == 0, (name, t, e, rc)  # lanes that replicate a value agree bit for bit
            q[e], v[e], w[e] = qo, vo, wo
            res["hash"][t, e] = np.frombuffer(hashlib.sha256(qo.tobytes() + vo.tobytes() + wo.tobytes()).digest()[:8], np.uint64)[0]
    return res


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_planar_lg_first_trip_host(lib, name):
    want = np.load(GOLDEN)
    got = _run(lib, name)
    # the recorded cases are the ones meant: the cap of one trip is reached, the cap of two is reached by fewer
    # envs, the pass that starts at the minimiser runs no trip at all
    assert want[f"{name}/cap1/iters"].max() == 1 and want[f"{name}/cap2/iters"].max() == 2
    assert (want[f"{name}/full/iters"] >= 2).any()
    assert (want[f"{name}/again/iters"] == 0).sum() > want[f"{name}/again/iters"].size // 2
    for key, g in got.items():
        w = want[f"{name}/{key}"]
        if key.endswith("iters") or key == "hash":
            bad = np.argwhere(g != w)
            assert bad.size == 0, (name, key, "first index that changed", bad[0].tolist())
        assert _same_bits(g, w), (name, key, "bits changed; first index",
                                  np.argwhere(g.view(np.uint64) != w.view(np.uint64))[0].tolist())


if __name__ == "__main__":
    if sys.argv[1] == "--write":
        L = _lib()
        out = {}
        for name in CONFIGS:
            r = _run(L, name)
            out.update({f"{name}/{k}": x for k, x in r.items()})
            print(name, {c: np.bincount(r[f"{c}/iters"].ravel()).tolist() for c in CASES})
        np.savez_compressed(GOLDEN, **out)
