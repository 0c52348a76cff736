"""Training of the PGX convolutional network, CPU side: the contract header envpool_amd/csrc/pgx_conv_train.hip.h built
for the host by g++ (tests/cpu_harness/pgx_conv_train_host.cpp) against the float64 twin `ConvNet.module()` with
autograd -- forward integers and saved bytes exactly, every gradient to float64 rounding, the crafted net that sits on
the clamps' boundaries --, and `module(kernels=True)` on CPU tensors: the twin's code, and the refusals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import pgx_conv_train_util as U
from envpool_amd.pgx.net import ConvNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"]
SRC = os.path.join(ROOT, "tests", "cpu_harness", "pgx_conv_train_host.cpp")
# (rows, H, W, C, D, L, P, A, shift_delta, net seed)
CASES = [(1, 3, 5, 3, 32, 0, 3, 9, 0, 0), (5, 3, 5, 3, 64, 1, 3, 9, -1, 0), (3, 4, 4, 2, 32, 2, 2, 40, 0, 105)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pgx_conv_train") / "libpgxconvtrainhost.so")
    subprocess.run(FLAGS + ["-shared", "-fPIC", SRC, "-o", out], check=True)
    return ctypes.CDLL(out)


def host_run(lib, net, x, dp, absolute=False):
    """(p, saved, g, [dW], [db]) of the header's by-the-book functions."""
    rows, n, (h, w, c) = len(x), len(net.layers), net.obs_shape
    ptrs = lambda arrays: (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrays])
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    wts, b = [l[0] for l in net.layers], [l[1] for l in net.layers]
    shifts = np.array([l[2] for l in net.layers], np.int32)
    saved = np.zeros((2 * net.blocks + 1, rows, h, w, net.channels), np.uint8)
    g = np.zeros((rows, h, w, net.planes), np.uint8)
    p = np.zeros((rows, net.actions + 1), np.int32)
    dw, db = [np.zeros(a.shape) for a in wts], [np.zeros(a.shape) for a in b]
    dp, x = np.ascontiguousarray(dp, np.float64), np.ascontiguousarray(x, np.uint8)
    rc = lib.pgx_conv_train_run(h, w, c, net.actions, net.channels, net.blocks, net.planes, rows, ptrs(wts), ptrs(b),
                                ptr(shifts), ptr(x), ptr(dp), int(absolute), ptr(saved), ptr(g), ptr(p), ptrs(dw),
                                ptrs(db))
    assert rc == 0
    return p, saved, g, dw, db


def check_against_twin(lib, net, x, seed):
    dp = np.random.default_rng(seed).standard_normal((len(x), net.actions + 1))
    want_p, want_dw, want_db = U.twin(net, x, dp)
    p, saved, g, dw, db = host_run(lib, net, x, dp)
    assert np.array_equal(p, want_p)
    pre, pre_g, _ = U.forward_np(net, x)
    for got, q in zip(list(saved) + [g], pre + [pre_g]):  # the activation, and bit 7 where the clamp changed it
        assert np.array_equal(got, np.clip(q, 0, 127) | (((q < 0) | (q > 127)) * 128))
    np_dw, np_db = U.backward_np(net, x, dp)
    abs_dw, abs_db = U.backward_np(net, x, dp, absolute=True)
    host_abs = host_run(lib, net, x, dp, absolute=True)
    for i in range(len(net.layers)):
        for got, want, mag in ((dw[i], want_dw[i], abs_dw[i]), (db[i], want_db[i], abs_db[i]),
                               (np_dw[i], want_dw[i], abs_dw[i]), (np_db[i], want_db[i], abs_db[i])):
            assert np.all(np.abs(got - want) <= 1e-12 * mag), i  # float64 rounding, relative to the sums' magnitudes
        assert np.allclose(host_abs[3][i], abs_dw[i], rtol=1e-12, atol=0)
        assert np.allclose(host_abs[4][i], abs_db[i], rtol=1e-12, atol=0)
    return want_dw


@pytest.mark.parametrize("case", CASES, ids=str)
def test_header_against_twin(lib, case):
    rows, h, w, c, d, blocks, planes, a, delta, seed = case
    net = ConvNet.random((h, w, c), a, d, blocks, planes, seed=seed, shift_delta=delta)
    want_dw = check_against_twin(lib, net, U.boards_of((h, w, c), rows), seed=1)
    assert all(np.any(g != 0) for g in want_dw)


def test_boundary_net(lib):
    """Values before a block's two clamps and the reduce layer's at exactly -1, 0, 127 and 128."""
    net, x = U.crafted()
    assert all(np.any(g != 0) for g in check_against_twin(lib, net, x, seed=2))


def test_slices(lib):
    """The slices cover the boards in whole passes, stay within the contract's counts and fit the workspace's."""
    out = (ctypes.c_int * 3)()
    for rows, h, w, n, k in ((1, 3, 5, 32, 3), (33, 3, 5, 64, 64), (70, 1, 1, 32, 32), (65536, 8, 8, 64, 64),
                             (2 ** 22, 1, 1, 32, 2), (32768, 8, 16, 256, 256), (34663, 11, 11, 32, 32)):
        lib.pgx_conv_train_slices(rows, h, w, n, k, out)
        assert out[0] * out[1] >= rows > (out[0] - 1) * out[1] and out[1] * h * w <= 8192 and out[0] <= 640
        for fewer in (rows, max(1, rows - 1), rows // 2 + 1):
            few = (ctypes.c_int * 3)()
            lib.pgx_conv_train_slices(fewer, h, w, n, k, few)
            assert few[0] <= out[2]


def test_kernels_flag_on_cpu_and_refusals(lib):
    net = ConvNet.random((3, 3, 2), 9, 32, 1, 2, seed=4)
    x = U.boards_of((3, 3, 2), 6)
    dp = np.random.default_rng(3).standard_normal((6, 10))
    plain, fast = U.twin(net, x, dp), U.twin(net, x, dp, kernels=True)
    assert np.array_equal(plain[0], fast[0])
    assert all(np.array_equal(a, b) for a, b in zip(plain[1] + plain[2], fast[1] + fast[2]))
    m = net.module(kernels=True)
    assert m.kernels and not net.module().kernels
    with pytest.raises(ValueError, match="must not require grad"):
        m.integers(torch.zeros((2, 18), dtype=torch.float64, requires_grad=True))
    with pytest.raises(ValueError, match="rows = 466034"):  # 2^22 / 9 = 466033
        m.integers(torch.zeros((466034, 18), dtype=torch.uint8))
    err = ctypes.create_string_buffer(240)
    for sizes, word in (((8, 17, 2, 9, 32, 1, 2, 4), "H = 8, W = 17"), ((3, 3, 33, 9, 32, 1, 2, 4), "C = 33"),
                        ((3, 3, 2, 128, 32, 1, 2, 4), "A = 128"), ((3, 3, 2, 9, 288, 1, 2, 4), "D = 288"),
                        ((3, 3, 2, 9, 32, 9, 2, 4), "L = 9"), ((8, 8, 2, 9, 32, 1, 9, 4), "P = 9"),
                        ((3, 3, 2, 9, 32, 1, 2, 0), "rows = 0"), ((3, 3, 2, 9, 32, 1, 2, 466034), "rows = 466034")):
        assert lib.pgx_conv_train_check(*sizes[:7], ctypes.c_longlong(sizes[7]), err, 240) == -1
        assert word in err.value.decode()
    assert lib.pgx_conv_train_check(8, 16, 32, 127, 256, 8, 4, ctypes.c_longlong(2 ** 15), err, 240) == 0
