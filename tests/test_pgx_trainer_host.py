"""The PGX trainer's contract without a GPU: csrc/pgx_trainer.hip.h built by g++ (cpu_harness/pgx_trainer_host.cpp):
the loss within kLossErr of the float64 restatement; update, norm and index hash equal to the numpy ones."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pgx_trainer_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"]
SRC = os.path.join(ROOT, "tests", "cpu_harness", "pgx_trainer_host.cpp")
ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pgx_trainer") / "libpgxtrainerhost.so")
    subprocess.run(FLAGS + ["-shared", "-fPIC", SRC, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.pgx_trainer_loss_err.restype = L.pgx_trainer_squares.restype = ctypes.c_double
    L.pgx_trainer_index.restype = ctypes.c_uint32
    L.pgx_trainer_index.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    L.pgx_trainer_loss.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_float] * 3 + \
        [ctypes.c_void_p] * 2
    L.pgx_trainer_update.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_double,
                                     ctypes.c_int] + [ctypes.c_void_p] * 4
    return L


@pytest.mark.parametrize("rows,a", [(1, 9), (33, 63), (7, 127)])
def test_loss_within_the_derived_bound(lib, rows, a):
    assert lib.pgx_trainer_loss_err() == U.LOSS_ERR
    rng = np.random.default_rng(rows)
    _, mask, pi, z = U.batch(rows, 4, a, seed=a)
    p = rng.integers(-60000, 60000, size=(rows, a + 1)).astype(np.int32)  # logits to +-20: e down to 1e-17
    scale_p, scale_v, vw = 1.0 / 3000.0, 1.0 / 50000.0, 0.5
    dp, row_loss = np.zeros((rows, a + 1), np.float32), np.zeros((rows, 2), np.float32)
    lib.pgx_trainer_loss(rows, a, ptr(p), ptr(mask), ptr(pi), ptr(z), scale_p, scale_v, vw, ptr(dp), ptr(row_loss))
    want, mag, pol, pol_mag, val = U.loss(p, mask, pi, z, scale_p, scale_v, vw)
    print(f"worst err / bound = {np.max(np.abs(dp - want) / np.maximum(U.LOSS_ERR * mag, 1e-300)):.3g}")
    assert np.all(np.abs(dp - want) <= U.LOSS_ERR * mag)
    assert want[:, :a].any()
    if rows > 1:  # row 0 has no legal action
        assert not dp[0, :a].any() and row_loss[0, 0] == 0.0
    assert abs(row_loss[:, 0].astype(np.float64).sum() / rows - pol) <= U.LOSS_ERR * pol_mag
    assert abs(row_loss[:, 1].astype(np.float64).sum() / rows - val) <= U.LOSS_ERR * val


@pytest.mark.parametrize("optimizer,clip", [("sgd", 0.0), ("adam", 0.0), ("sgd", 20.0)])
def test_update_norm_and_quantising_are_the_restatement(lib, optimizer, clip):
    rng = np.random.default_rng(5)
    count = 2 * U.CHUNK
    masters = [rng.integers(-127, 128, size=count - 3).astype(np.float64)]
    rule = U.Rule(masters, optimizer, lr=1.5, momentum=0.9, weight_decay=1e-3, clip=clip)
    master, s1, s2 = masters[0].copy(), np.zeros(count - 3), np.zeros(count - 3)
    pow1 = pow2 = 1.0
    for step in range(2):
        grad = rng.standard_normal(count - 3).astype(np.float32)
        padded = np.zeros(count, np.float32)
        padded[:count - 3] = grad
        norm = np.sqrt(lib.pgx_trainer_squares(ptr(padded), count))
        assert norm == rule.step([grad]) and (clip == 0.0 or norm > clip)  # (the clip bites)
        pow1, pow2 = pow1 * 0.9, pow2 * 0.999
        r = np.array([optimizer == "adam", 1.5, 0.9, 0.9, 0.999, 1.0 - 0.9, 1.0 - 0.999,
                      1.5 * np.sqrt(1.0 - pow2) / (1.0 - pow1), 1e-8, 1e-3], np.float64)
        q = np.zeros(count - 3, np.int32)
        lib.pgx_trainer_update(ptr(r), count - 3, ptr(grad), clip, norm, 1, ptr(master), ptr(s1), ptr(s2), ptr(q))
        assert np.array_equal(master, rule.master[0]) and np.array_equal(s1, rule.s1[0])
        assert optimizer == "sgd" or np.array_equal(s2, rule.s2[0])
        assert np.array_equal(q, rule.quantised(0, True))
    assert (np.abs(q) == 127).any() and (q != masters[0]).any()


def test_index_hash(lib):
    for seed, t, j, count in [(0, 0, 0, 1), (7, 3, 32, 50), (2 ** 63 + 5, 2 ** 31 + 1, 4095, 2 ** 32 - 1)]:
        got = lib.pgx_trainer_index(seed, t, j, count)
        assert got == U.index(seed, t, j, count) and got < count
