"""PGX convolutional network, CPU side: envpool_amd/csrc/pgx_conv.hip.h built by g++ against the numpy restatement
(pgx_conv_util.py), bit for bit; the torch twin and the way back; the blob, save / load; ConvParse's refusals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pgx_conv_util as U
from envpool_amd.pgx.net import ConvNet
from pgx_net_util import bits, random_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"]
SRC = os.path.join(ROOT, "tests", "cpu_harness", "pgx_conv_host.cpp")
SMALL = (3, 3, 2, 9, 32, 1, 4)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pgx_conv") / "libpgxconvhost.so")
    subprocess.run(FLAGS + ["-shared", "-fPIC", SRC, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.pgx_conv_blob_bytes.restype = ctypes.c_size_t
    return L


_ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

def parse_error(lib, blob, dense=False):
    err = ctypes.create_string_buffer(256)
    rc = (lib.pgx_conv_dense_parse if dense else lib.pgx_conv_parse)(_ptr(blob), ctypes.c_size_t(blob.nbytes), err, 256)
    return rc, err.value.decode()


def case_net(case, seed=0, shift_delta=0):
    layers = U.random_layers(*case, seed, shift_delta)
    sp, sv = U.scales(case[0], case[1], case[6])
    return layers, sp, sv, U.make_blob(*case, layers, sp, sv)


@pytest.mark.parametrize("case", U.ALL, ids=str)
def test_header_against_numpy(lib, case):
    delta, case = case[7], case[:7]
    h, w, c, a, d, blocks, p = case
    layers, sp, sv, blob = case_net(case, U.SEEDS[case], delta)
    assert blob.nbytes == lib.pgx_conv_blob_bytes(*case)
    for rows in U.ROWS:
        obs, mask, status = random_rows(h * w * c, a, rows, seed=rows)
        if rows == 100:
            U.check_spread(layers, blocks, (h, w, c), obs, lowered=delta != 0)
        for priors in (False, True):
            want = U.restate(layers, blocks, (h, w, c), sp, sv, obs, mask, status, priors)
            policy, value = np.empty((rows, a), np.float32), np.empty(rows, np.float32)
            assert lib.pgx_conv_eval(_ptr(blob), ctypes.c_size_t(blob.nbytes), rows, int(priors), _ptr(obs), _ptr(mask),
                                     _ptr(status), _ptr(policy), _ptr(value)) == 0
            assert np.array_equal(bits(policy), bits(want[0])), (case, rows, priors)
            assert np.array_equal(bits(value), bits(want[1])), (case, rows, priors)


def test_class_blob_save_load(tmp_path):
    case = (6, 7, 2, 7, 64, 1, 4)
    layers, sp, sv, blob = case_net(case, seed=3)
    net = ConvNet((6, 7, 2), 7, 64, 1, 4, layers, sp, sv)
    assert np.array_equal(net.blob(), blob) and net.inputs == 84 and net._is_epa_net
    path = str(tmp_path / "c4.npz")
    net.save(path)
    for other in (ConvNet.from_blob(blob), ConvNet.load(path), ConvNet.random((6, 7, 2), 7, 64, 1, 4, seed=3)):
        assert np.array_equal(other.blob(), blob) and other.obs_shape == (6, 7, 2)


@pytest.mark.parametrize("case", [SMALL, (6, 7, 2, 7, 64, 1, 4), (8, 8, 2, 65, 64, 2, 8)], ids=str)
def test_module_against_numpy_and_back(case):
    import torch
    h, w, c, a, d, blocks, p = case
    layers, sp, sv, blob = case_net(case, seed=7)
    m = ConvNet((h, w, c), a, d, blocks, p, layers, sp, sv).module()
    obs, mask, _ = random_rows(h * w * c, a, 33, seed=5)
    want_p, _ = U.integers(layers, blocks, (h, w, c), obs)
    x = torch.tensor(obs.astype(np.float64), requires_grad=True)
    got = m.integers(x)
    assert got.dtype == torch.float64 and np.array_equal(got.detach().numpy(), want_p.astype(np.float64))
    logits, value = m(x)
    want = U.restate(layers, blocks, (h, w, c), sp, sv, obs, mask, np.zeros(33, np.uint8), False)
    assert np.array_equal(bits(logits.detach().numpy()), bits(want[0]))
    assert np.array_equal(bits(value.detach().numpy()), bits(want[1]))
    got.sum().backward()  # straight-through: every layer's weights get a gradient
    assert all(wt.grad is not None and bool((wt.grad != 0).any()) for wt in m.weights)
    assert np.array_equal(ConvNet.from_module(m).blob(), blob)


def _refusals():
    layers, sp, sv, good = case_net(SMALL)

    def sized(**kw):
        sizes = dict(zip("hwcadlp", SMALL), **kw)
        return U.make_blob(*(sizes[k] for k in "hwcadlp"), layers, sp, sv)

    def with_layer(i, at, value):
        ls = [list(x) for x in layers]
        if at == 2:
            ls[i][2] = value
        else:
            ls[i][at] = ls[i][at].copy()
            ls[i][at].reshape(-1)[1] = value
        return U.make_blob(*SMALL, [tuple(x) for x in ls], sp, sv)

    return good, [
        (sized(h=0), "conv: H = 0, W = 3 must be at least 1 with H W <= 128"),
        (sized(h=12, w=11), "conv: H = 12, W = 11 must be at least 1 with H W <= 128"),
        (sized(c=33), "conv: C = 33 must be 1 .. 32"),
        (sized(a=128), "conv: A = 128 must be 1 .. 127"),
        (sized(d=48), "conv: D = 48 must be a multiple of 32 in 32 .. 256"),
        (sized(l=9), "conv: L = 9 must be 0 .. 8"),
        (sized(p=33), "conv: P = 33 must be 1 .. 32 with H W P <= 512"),
        (sized(h=8, w=8, p=9), "conv: P = 9 must be 1 .. 32 with H W P <= 512"),
        (with_layer(1, 0, -128), "conv: layer 1: a weight of -128 (weights are -127 .. 127)"),
        (with_layer(3, 1, (1 << 30) + 1), "conv: layer 3: a bias of 1073741825 is past 2^30 in magnitude"),
        (with_layer(0, 2, 25), "conv: layer 0: shift = 25 must be 0 .. 24"),
        (with_layer(4, 2, 1), "conv: layer 4: shift = 1 must be 0 .. 0"),
        (U.make_blob(*SMALL, layers, 0.0, sv), "conv: scale_p must be finite, above 0 and at most 1e20"),
        (U.make_blob(*SMALL, layers, sp, sv, version=2), "conv: version = 2 must be 1"),
        (U.make_blob(*SMALL, layers, sp, sv, magic=0x4E584750), "conv: the blob does not begin with the magic PGXC"),
        (good[:40], "conv: a blob of 40 bytes is shorter than a header"),
        (good[:-4].copy(), f"conv: a blob of {good.nbytes - 4} bytes for a network of {good.nbytes} bytes"),
        (np.concatenate([good, np.zeros(4, np.uint8)]),
         f"conv: a blob of {good.nbytes + 4} bytes for a network of {good.nbytes} bytes"),
    ]


GOOD, REFUSALS = _refusals()


@pytest.mark.parametrize("blob,message", REFUSALS, ids=[m[:48] for _, m in REFUSALS])
def test_parse_refusals(lib, blob, message):
    assert parse_error(lib, GOOD) == (0, "")
    rc, got = parse_error(lib, blob)
    assert rc == -1 and got.startswith(message), got


def test_the_dense_parse_and_the_class_refuse(lib):
    layers, sp, sv, good = case_net(SMALL)
    assert parse_error(lib, good, dense=True) == (-1, "net: the blob does not begin with the magic PGXN")
    w128 = layers[1][0].copy()
    w128[5, 1, 1, 7] = -128
    with pytest.raises(ValueError, match=r"conv: layer 1: a weight of -128 \(weights are -127 \.\. 127\)"):
        ConvNet((3, 3, 2), 9, 32, 1, 4, [(w128 if i == 1 else w, b, s) for i, (w, b, s) in enumerate(layers)], sp, sv)
