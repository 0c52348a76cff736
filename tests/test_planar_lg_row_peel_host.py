"""Bit-identity pin, on the CPU, of the pass over the constraint rows of the lane-group planar step (plg::RowsPass) whose
first end-sphere visit WRITES most of the Hessian accumulators (kPeel: code of its own in front of the slot loop, groups
of two lanes) where every other visit adds to accumulators zeroed in front of the loop.  The host instantiation of the
kernel source (tests/cpu_harness/planar_lg_row_peel_host.cpp over planar_lg_host.cpp and
envpool_amd/csrc/mj_planar_lg.hip.h) runs single forward passes at crafted states, pools of 2 and 3 envs each:

  air       the robot hangs above the floor, every hinge inside its range: no slot touches on any lane, the limit rows
            alone write (zero weights) and the caller's zeros stay
  limit     in the air with one hinge beyond its range: a limit row is active with no contact
  one       exactly one lane touches, one slot: the other lanes take the first visit on the sentinel record
  two       a lane touches two slots or more: the first visit is followed by visits of the loop
  zeros     every angle exactly zero (HalfCheetah: and the feet in the floor): Jacobian columns that are exactly +-0 (the
            Walker2d's foot end stands exactly under its hinges: Jn = -(x - x) = -0), tangential velocity of either sign
            so that the friction rows' Bc = mu (w3 - w2) takes either sign and the products with those columns are +0
            and -0

for HalfCheetah and Walker2d on groups of 2 and 4 lanes.  Per lane qacc, the gradient, the trip counts, the own slot
sets and the per-trip active-row masks are compared for exact equality with tests/golden/planar_lg_row_peel_host.npz;
the lanes' parts of H after every pass over the rows are compared as NUMBERS (-0.0 == +0.0: a written entry may hold
-0.0 where an accumulated one holds +0.0, which is the point of the argument in RowsPass -- it must reach no result).

The golden file was recorded with the sources of the parent commit of the change that added this file (plus the
no-op hook that hands the masks out).  The values are the host's (x86-64, no FMA contraction): this pins the control
flow and the operation order of the source; tests/test_gpu_planar_lg_row_peel.py pins the device build.

Regenerate (only when the arithmetic is meant to change):  python tests/test_planar_lg_row_peel_host.py --write
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "planar_lg_row_peel_host.npz")
HARNESS = os.path.join(ROOT, "tests", "cpu_harness")
CSRC = os.path.join(ROOT, "envpool_amd", "csrc")
KLV, KTRI, REC_TRIPS = 6, 21, 16
# name -> (model of the harness, lanes per env, rootz of the reset pose, a hinge angle beyond the first hinge's range)
CONFIGS = {
    "HalfCheetah-kl2": (0, 2, 0.0, 1.3),
    "HalfCheetah-kl4": (0, 4, 0.0, 1.3),
    "Walker2d-kl2": (1, 2, 1.25, 0.3),
    "Walker2d-kl4": (1, 4, 1.25, 0.3),
}
# scenario -> per model (HalfCheetah, Walker2d): (pitch, height above the reset pose, angle of the second leg's first
# hinge); found by lowering the robot in steps of 0.01 until the lanes' slot sets are the ones the scenario names
SCENARIOS = {
    "air": ((0.0, 0.3, 0.0), (0.0, 0.3, 0.0)),
    "limit": ((0.0, 0.3, 0.0), (0.0, 0.3, 0.0)),
    "one": ((0.0, -0.09, 0.0), (0.3, -0.05, -0.9)),
    "two": ((0.3, -0.2, 0.0), (0.0, -0.08, 0.0)),
    "zeros": ((0.0, -0.12, 0.0), (0.0, -0.05, 0.0)),
}
# envs of a scenario: torso velocity (x, z, pitch rate); pools of 2 and of 3
VELS = {
    "air": ((0.5, 0.0, 0.0), (-0.5, 0.2, 0.1)),
    "limit": ((0.5, 0.0, 0.0), (-0.5, 0.2, 0.1), (0.0, 0.0, 0.0)),
    "one": ((0.5, 0.0, 0.0), (-0.5, -0.3, 0.0)),
    "two": ((0.5, 0.0, 0.0), (-0.5, -0.3, 0.2), (0.0, -1.0, 0.0)),
    "zeros": ((0.5, 0.0, 0.0), (-0.5, 0.0, 0.0), (0.0, 0.0, 0.0)),
}


def _lib():
    so, src = os.path.join(HARNESS, "libplanar_lg_row_peel_host.so"), os.path.join(HARNESS, "planar_lg_row_peel_host.cpp")
    deps = [src, os.path.join(HARNESS, "planar_lg_host.cpp")] + [os.path.join(CSRC, x) for x in
                                                                ("mj_planar_lg.hip.h", "mj_cheetah.hip.h", "mj_cheetah_model.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", src, "-o", so], check=True)
    L = ctypes.CDLL(so)
    L.planar_lg_rows.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 11
    L.planar_lg_rows.restype = None
    return L


@pytest.fixture(scope="module")
def lib():
    return _lib()


def _run(L, name):
    """{scenario/key: array over the scenario's envs}"""
    model, kl, z0, beyond = CONFIGS[name]
    res = {}
    for sc, per_model in SCENARIOS.items():
        pitch, dz, hinge = per_model[0 if model == 0 else 1]
        n = len(VELS[sc])
        out = {"qacc": np.zeros((n, KLV, kl)), "grad": np.zeros((n, KLV, kl)), "iters": np.zeros((n, kl), np.int32),
               "own": np.zeros((n, kl), np.uint32), "trips": np.zeros(n, np.int32),
               "masks": np.zeros((n, REC_TRIPS, kl), np.uint32), "h": np.zeros((n, REC_TRIPS, KTRI, kl))}
        for e, vel in enumerate(VELS[sc]):
            q, v, w, a = np.zeros(9), np.zeros(9), np.zeros(9), np.zeros(6)
            q[1], q[2], q[6] = z0 + dz, pitch, hinge
            if sc == "limit":
                q[3] = beyond
            v[:3] = vel
            trips = ctypes.c_int(0)
            L.planar_lg_rows(model, kl, q.ctypes.data, v.ctypes.data, w.ctypes.data, a.ctypes.data,
                             out["qacc"][e].ctypes.data, out["grad"][e].ctypes.data, out["iters"][e].ctypes.data,
                             out["own"][e].ctypes.data, ctypes.byref(trips), out["masks"][e].ctypes.data,
                             out["h"][e].ctypes.data)
            out["trips"][e] = trips.value
        res.update({f"{sc}/{k}": x for k, x in out.items()})
    return res


def _slots(own):
    """touching slots per lane"""
    return np.array([[bin(int(x)).count("1") for x in row] for row in own])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_planar_lg_row_peel_host(lib, name):
    want = np.load(GOLDEN)
    g = lambda key: want[f"{name}/{key}"]  # noqa: E731
    # the recorded states are the ones meant
    for sc in ("air", "limit"):
        assert not g(f"{sc}/own").any(), (name, sc, "a slot touches")
    assert not g("air/masks").any() and (g("limit/masks")[:, 0] & 7).any(), (name, "limit rows")
    assert (_slots(g("one/own")).sum(axis=1) == 1).all(), (name, "one", _slots(g("one/own")).tolist())
    assert (_slots(g("two/own")).max(axis=1) >= 2).all(), (name, "two", _slots(g("two/own")).tolist())
    assert (_slots(g("zeros/own")).max(axis=1) >= 1).all() and (g("zeros/h") == 0).any(), (name, "zeros")
    assert max(g(f"{sc}/trips").max() for sc in SCENARIOS) <= REC_TRIPS
    got = _run(lib, name)
    for key, x in got.items():
        w = g(key)
        if key.endswith("/h"):
            assert x.shape == w.shape and np.array_equal(x, w), (name, key, "H changed as numbers")
            continue
        if x.dtype != np.float64:
            bad = np.argwhere(x != w)
            assert bad.size == 0, (name, key, "first index that changed", bad[0].tolist())
        assert _same_bits(x, w), (name, key, "bits changed; first index",
                                  np.argwhere(x.view(np.uint64) != w.view(np.uint64))[0].tolist())


if __name__ == "__main__":
    if sys.argv[1] == "--write":
        L = _lib()
        out = {}
        for name in CONFIGS:
            r = _run(L, name)
            out.update({f"{name}/{k}": x for k, x in r.items()})
            print(name, {sc: (_slots(r[f"{sc}/own"]).tolist(), r[f"{sc}/trips"].tolist()) for sc in SCENARIOS})
        np.savez_compressed(GOLDEN, **out)
