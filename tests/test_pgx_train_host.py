"""Training of the PGX built-in network, CPU side: the contract header envpool_amd/csrc/pgx_train.hip.h built for the
host by g++ (tests/cpu_harness/pgx_train_host.cpp) against the float64 twin `Net.module()` with autograd -- forward
integers exactly, every gradient to float64 rounding, the crafted net that sits on the clamps' boundaries --, and
`module(kernels=True)` on CPU tensors: the twin's code, and the refusals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import pgx_train_util as U
from envpool_amd.actor import Actor
from envpool_amd.pgx.net import Net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"]
SRC = os.path.join(ROOT, "tests", "cpu_harness", "pgx_train_host.cpp")
# (rows, F, D, L, A, binary inputs, shift_delta)
CASES = [(5, 18, 32, 0, 9, True, 0), (33, 84, 96, 1, 65, False, 0), (7, 40, 64, 2, 127, True, -2)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pgx_train") / "libpgxtrainhost.so")
    subprocess.run(FLAGS + ["-shared", "-fPIC", SRC, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.pgx_train_split_join.restype = ctypes.c_float
    L.pgx_train_split_join.argtypes = [ctypes.c_float]
    return L


def host_run(lib, net, x, dp, absolute=False):
    """(p, saved, [dW], [db]) of the header's by-the-book functions."""
    rows, n = len(x), len(net.layers)
    ptrs = lambda arrays: (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrays])
    w, b = [l[0] for l in net.layers], [l[1] for l in net.layers]
    shifts = np.array([l[2] for l in net.layers], np.int32)
    saved = np.zeros((2 * net.blocks + 1, rows, net.hidden), np.uint8)
    p = np.zeros((rows, net.actions + 1), np.int32)
    dw, db = [np.zeros(a.shape) for a in w], [np.zeros(a.shape) for a in b]
    dp = np.ascontiguousarray(dp, np.float64)
    rc = lib.pgx_train_run(net.inputs, net.actions, net.hidden, net.blocks, rows, ptrs(w), ptrs(b),
                           shifts.ctypes.data_as(ctypes.c_void_p), x.ctypes.data_as(ctypes.c_void_p),
                           dp.ctypes.data_as(ctypes.c_void_p), int(absolute), saved.ctypes.data_as(ctypes.c_void_p),
                           p.ctypes.data_as(ctypes.c_void_p), ptrs(dw), ptrs(db))
    assert rc == 0
    return p, saved, dw, db


def check_against_twin(lib, net, x, seed):
    dp = np.random.default_rng(seed).standard_normal((len(x), net.actions + 1))
    want_p, want_dw, want_db = U.twin(net, x, dp)
    p, saved, dw, db = host_run(lib, net, x, dp)
    assert np.array_equal(p, want_p)
    pre, _ = U.forward_np(net, x)
    for j, q in enumerate(pre):  # the saved bytes: the activation, and bit 7 where the clamp changed it
        assert np.array_equal(saved[j], np.clip(q, 0, 127) | (((q < 0) | (q > 127)) * 128))
    np_dw, np_db = U.backward_np(net, x, dp)
    abs_dw, abs_db = U.backward_np(net, x, dp, absolute=True)
    host_abs = host_run(lib, net, x, dp, absolute=True)
    for i in range(len(net.layers)):
        for got, want, mag in ((dw[i], want_dw[i], abs_dw[i]), (db[i], want_db[i], abs_db[i]),
                               (np_dw[i], want_dw[i], abs_dw[i]), (np_db[i], want_db[i], abs_db[i])):
            assert np.all(np.abs(got - want) <= 1e-12 * mag), i  # float64 rounding, relative to the sums' magnitudes
            assert np.all(mag[want != 0] > 0)  # G_abs is nonzero wherever the gradient is
        assert np.allclose(host_abs[2][i], abs_dw[i], rtol=1e-12, atol=0)
        assert np.allclose(host_abs[3][i], abs_db[i], rtol=1e-12, atol=0)
    return want_dw


@pytest.mark.parametrize("case", CASES, ids=str)
def test_header_against_twin(lib, case):
    rows, f, d, blocks, a, binary, delta = case
    net = Net.random((f,), a, d, blocks, seed=rows, shift_delta=delta)
    want_dw = check_against_twin(lib, net, U.rows_of(f, rows, 3, binary), seed=1)
    assert all(np.any(g != 0) for g in want_dw)


def test_boundary_net(lib):
    """Values before both clamps of a block at exactly -1, 0, 127 and 128: the inclusive mask and the residual split."""
    net, x = U.crafted()
    want_dw = check_against_twin(lib, net, x, seed=2)
    # row 0 alone: the gradient passes the clamps at 0 and 127, and not at -1 and 128
    _, dw, _ = U.twin(net, x[:1], np.ones((1, 4)))
    head = net.layers[3][0].astype(np.float64).sum(axis=0)
    assert np.array_equal(dw[1][:4, 2] != 0, [False, True, True, False]) and dw[1][2, 2] == 127 * head[2]
    assert np.array_equal(dw[2][4:8, 6] != 0, [False, True, True, False])
    assert want_dw[0].any()


def test_split_and_slices(lib):
    """hi + lo is within 2^-16 of the value; the slices cover the rows in whole runs and fit the workspace's count."""
    for v in np.random.default_rng(0).standard_normal(200).astype(np.float32) * np.float32(1e3):
        assert abs(float(lib.pgx_train_split_join(float(v))) - float(v)) <= 2.0 ** -16 * abs(float(v))
    out = (ctypes.c_int * 3)()
    for rows, n, k in ((1, 10, 32), (130, 32, 18), (4096, 128, 128), (65536, 512, 513), (65537, 32, 32), (1 << 20, 66, 512)):
        lib.pgx_train_slices(rows, n, k, out)
        assert out[0] * out[1] >= rows > (out[0] - 1) * out[1] and out[1] % 128 == 0 and out[1] <= 8192
        for fewer in (rows, max(1, rows - 1), rows // 2 + 1):
            few = (ctypes.c_int * 3)()
            lib.pgx_train_slices(fewer, n, k, few)
            assert few[0] <= out[2]


def test_kernels_flag_on_cpu():
    """`kernels=True` on CPU tensors is the twin's code, for a Net and for an Actor's trunk."""
    net = Net.random((18,), 9, 32, 1, seed=4)
    x = U.rows_of(18, 6, 1, False)
    dp = np.random.default_rng(3).standard_normal((6, 10))
    plain, fast = U.twin(net, x, dp), U.twin(net, x, dp, kernels=True)
    assert np.array_equal(plain[0], fast[0])
    assert all(np.array_equal(a, b) for a, b in zip(plain[1] + plain[2], fast[1] + fast[2]))
    actor = Actor.random(dict(features=5, kind=0, actions=3, low=np.zeros(0, np.float32), high=np.zeros(0, np.float32),
                              obs_low=np.full(5, -1.0), obs_high=np.full(5, 1.0)), hidden=32, blocks=1, seed=1)
    obs = torch.tensor(np.random.default_rng(1).uniform(-1, 1, (4, 5)))
    assert actor.module(kernels=True).net.kernels and not actor.module().net.kernels
    fast, plain = actor.module(kernels=True), actor.module()
    assert torch.equal(fast.integers(obs), plain.integers(obs))
    action = torch.tensor([0, 2, 1, 1])
    assert torch.equal(fast.logp_of(fast(obs)[0], action), plain.logp(obs, action))  # one pass for both heads
    # an input outside the contract's integers 0 .. 127 is rounded half to even and clamped, as the kernels read it
    odd = torch.tensor([[-3.0, 0.5, 1.5, 126.5, 127.4, 300.0, float("nan")] + [2.0] * 11], dtype=torch.float64)
    want = torch.tensor([[0.0, 0.0, 2.0, 126.0, 127.0, 127.0, 0.0] + [2.0] * 11], dtype=torch.float64)
    assert torch.equal(net.module(kernels=True).integers(odd), net.module().integers(want))


def test_refusals(lib):
    m = Net.random((18,), 9, 32, 1, seed=4).module(kernels=True)
    with pytest.raises(ValueError, match="must not require grad"):
        m.integers(torch.zeros((2, 18), dtype=torch.float64, requires_grad=True))
    with pytest.raises(ValueError, match="rows = 1048577"):
        m.integers(torch.zeros((2 ** 20 + 1, 18), dtype=torch.uint8))
    with pytest.raises(ValueError, match="rows = 0"):
        m.integers(torch.zeros((0, 18)))
    err = ctypes.create_string_buffer(200)
    for sizes, word in (((0, 9, 32, 1, 4), "F = 0"), ((513, 9, 32, 1, 4), "F = 513"), ((18, 128, 32, 1, 4), "A = 128"),
                        ((18, 9, 48, 1, 4), "D = 48"), ((18, 9, 544, 1, 4), "D = 544"), ((18, 9, 32, 9, 4), "L = 9"),
                        ((18, 9, 32, 1, 0), "rows = 0"), ((18, 9, 32, 1, 2 ** 20 + 1), "rows = 1048577")):
        assert lib.pgx_train_check(*sizes[:4], ctypes.c_longlong(sizes[4]), err, 200) == -1
        assert word in err.value.decode()
    assert lib.pgx_train_check(512, 127, 512, 8, ctypes.c_longlong(2 ** 20), err, 200) == 0
