"""PGX built-in network, CPU side: the contract header envpool_amd/csrc/pgx_net.hip.h built for the host by g++
(tests/cpu_harness/pgx_net_host.cpp) against the numpy restatement (pgx_net_util.py), bit for bit, in both modes; the
torch twin `Net.module()` against the same restatement and the way back; save / load and the blob; the refusals of a
blob that is no network, each with its message; and the session methods' `run(net)` on a stand-in pool."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pgx_net_util as U
from envpool_amd.core import native
from envpool_amd.pgx.net import Net
from envpool_amd.python.envpool import GuidedSearch, GumbelSearch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"]  # no fast-math, no contraction
SRC = os.path.join(ROOT, "tests", "cpu_harness", "pgx_net_host.cpp")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pgx_net") / "libpgxnethost.so")
    subprocess.run(FLAGS + ["-shared", "-fPIC", SRC, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.pgx_net_blob_bytes.restype = ctypes.c_size_t
    return L


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_eval(lib, blob, f, a, obs, mask, status, priors):
    rows = len(status)
    policy, value = np.empty((rows, a), np.float32), np.empty(rows, np.float32)
    rc = lib.pgx_net_eval(_ptr(blob), ctypes.c_size_t(blob.nbytes), rows, 1 if priors else 0, _ptr(obs), _ptr(mask),
                          _ptr(status), _ptr(policy), _ptr(value))
    assert rc == 0
    return policy, value


def parse_error(lib, blob):
    err = ctypes.create_string_buffer(256)
    rc = lib.pgx_net_parse(_ptr(blob), ctypes.c_size_t(blob.nbytes), err, 256)
    return rc, err.value.decode()


def case_net(case, seed=0, shift_delta=0):
    f, a, d, blocks = case
    layers = U.random_layers(f, a, d, blocks, seed, shift_delta)
    sp, sv = U.scales(d)
    return layers, sp, sv, U.make_blob(f, a, d, blocks, layers, sp, sv)


@pytest.mark.parametrize("case", U.CASES + [U.LOWERED + (-2,)], ids=str)
def test_header_against_numpy(lib, case):
    """Logits and priors modes, rows 1, 31, 33 and 100, statuses 0 / 1 / 2, masks with a single legal action; the last
    case lowers every shift by 2 so that the upper clamp is common."""
    delta = case[4] if len(case) == 5 else 0
    f, a, d, blocks = case[:4]
    layers, sp, sv, blob = case_net(case[:4], seed=U.SEEDS[case[:4]], shift_delta=delta)
    assert blob.nbytes == lib.pgx_net_blob_bytes(f, a, d, blocks)
    for rows in U.ROWS:
        obs, mask, status = U.random_rows(f, a, rows, seed=rows)
        if rows == 100:
            U.check_spread(layers, blocks, obs, lowered=delta != 0)
        assert rows < 5 or ((mask.sum(axis=1) == 1).any() and len(set(status.tolist())) == 3)
        for priors in (False, True):
            want = U.restate(layers, blocks, sp, sv, obs, mask, status, priors)
            got = host_eval(lib, blob, f, a, obs, mask, status, priors)
            assert np.array_equal(U.bits(got[0]), U.bits(want[0])), (case, rows, priors)
            assert np.array_equal(U.bits(got[1]), U.bits(want[1])), (case, rows, priors)
            if priors:
                live = status == 0
                assert np.allclose(got[0][live].sum(axis=1), 1.0, atol=1e-5)
                assert not got[0][mask == 0].any() and not got[0][~live].any() and not got[1][~live].any()


def test_net_class_blob_save_load(tmp_path):
    f, a, d, blocks = 84, 7, 64, 1
    layers, sp, sv, blob = case_net((f, a, d, blocks), seed=3)
    net = Net((6, 7, 2), a, d, blocks, layers, sp, sv)
    assert np.array_equal(net.blob(), blob)  # the class writes the blob the hand-made one is
    back = Net.from_blob(blob, (6, 7, 2))
    path = str(tmp_path / "c4.npz")
    net.save(path)
    loaded = Net.load(path)
    for other in (back, loaded):
        assert np.array_equal(other.blob(), blob) and other.obs_shape == (6, 7, 2)
    # Net.random is the recipe of the tests
    rnd = Net.random((6, 7, 2), a, d, blocks, seed=3)
    assert np.array_equal(rnd.blob(), blob)
    assert not np.array_equal(Net.random((6, 7, 2), a, d, blocks, seed=4).blob(), blob)


@pytest.mark.parametrize("case", [(18, 9, 32, 0), (84, 7, 64, 1), (128, 65, 128, 2)], ids=str)
def test_module_against_numpy_and_back(case):
    import torch
    f, a, d, blocks = case
    layers, sp, sv, blob = case_net(case, seed=7)
    net = Net((f,), a, d, blocks, layers, sp, sv)
    m = net.module()
    obs, mask, status = U.random_rows(f, a, 33, seed=5)
    p, _ = U.integers(layers, blocks, obs)
    x = torch.tensor(obs.astype(np.float64), requires_grad=True)
    got = m.integers(x)
    assert got.dtype == torch.float64 and np.array_equal(got.detach().numpy(), p.astype(np.float64))
    logits, value = m(x)
    want = U.restate(layers, blocks, sp, sv, obs, mask, np.zeros(33, np.uint8), False)
    assert np.array_equal(U.bits(logits.detach().numpy()), U.bits(want[0]))
    assert np.array_equal(U.bits(value.detach().numpy()), U.bits(want[1]))
    # straight-through: the rounding passes a gradient to every layer's weights
    got.sum().backward()
    assert all(w.grad is not None and bool((w.grad != 0).any()) for w in m.weights)
    assert np.array_equal(Net.from_module(m).blob(), blob)


def test_parse_refusals(lib):
    f, a, d, blocks = 18, 9, 32, 1
    layers, sp, sv, good = case_net((f, a, d, blocks))
    assert parse_error(lib, good) == (0, "")

    def with_layer(i, w=None, b=None, shift=None):
        ls = [list(x) for x in layers]
        if w is not None:
            ls[i][0] = w
        if b is not None:
            ls[i][1] = b
        if shift is not None:
            ls[i][2] = shift
        return U.make_blob(f, a, d, blocks, [tuple(x) for x in ls], sp, sv)

    w128 = layers[1][0].copy()
    w128[5, 7] = -128
    bias = layers[2][1].copy()
    bias[3] = (1 << 30) + 1
    cases = [
        (U.make_blob(f, a, 48, blocks, layers, sp, sv), "net: D = 48 must be a multiple of 32 in 32 .. 512"),
        (U.make_blob(f, a, 544, blocks, layers, sp, sv), "net: D = 544 must be a multiple of 32 in 32 .. 512"),
        (U.make_blob(f, a, d, 9, layers, sp, sv), "net: L = 9 must be 0 .. 8"),
        (U.make_blob(f, a, d, -1, layers, sp, sv), "net: L = -1 must be 0 .. 8"),
        (with_layer(0, shift=25), "net: layer 0: shift = 25 must be 0 .. 24"),
        (with_layer(3, shift=1), "net: layer 3: shift = 1 must be 0 .. 0"),
        (with_layer(1, w=w128), "net: layer 1: a weight of -128 (weights are -127 .. 127)"),
        (with_layer(2, b=bias), "net: layer 2: a bias of 1073741825 is past 2^30 in magnitude"),
        (U.make_blob(f, a, d, blocks, layers, sp, sv, magic=1), "net: the blob does not begin with the magic PGXN"),
        (U.make_blob(f, a, d, blocks, layers, sp, sv, version=2), "net: version = 2 must be 1"),
        (U.make_blob(f, a, d, blocks, layers, 0.0, sv), "net: scale_p must be finite, above 0 and at most 1e20"),
        (U.make_blob(f, a, d, blocks, layers, sp, float("nan")), "net: scale_v must be finite, above 0 and at most 1e20"),
        (U.make_blob(600, a, d, blocks, layers, sp, sv), "net: F = 600 must be 1 .. 512"),
        (U.make_blob(f, 128, d, blocks, layers, sp, sv), "net: A = 128 must be 1 .. 127"),
        (good[:20], "net: a blob of 20 bytes is shorter than a header"),
    ]
    for blob, message in cases:
        assert parse_error(lib, blob) == (-1, message)
    rc, message = parse_error(lib, good[:-4].copy())
    assert rc == -1 and message.startswith(f"net: a blob of {good.nbytes - 4} bytes for a network of {good.nbytes} bytes")
    # the class refuses the same nets before any native call, with the same words
    with pytest.raises(ValueError, match=r"a weight of -128 \(weights are -127 \.\. 127\)"):
        Net((f,), a, d, blocks, [(w128 if i == 1 else w, b, s) for i, (w, b, s) in enumerate(layers)], sp, sv)
    with pytest.raises(ValueError, match="a bias of 1073741825 is past 2\\^30"):
        Net((f,), a, d, blocks, [(w, bias if i == 2 else b, s) for i, (w, b, s) in enumerate(layers)], sp, sv)
    with pytest.raises(ValueError, match="D = 48 must be a multiple of 32"):
        Net((f,), a, 48, blocks, layers, sp, sv)
    with pytest.raises(ValueError, match="L = 9 must be 0 .. 8"):
        Net((f,), a, d, 9, layers, sp, sv)
    with pytest.raises(ValueError, match="layer 0: shift = 25 must be 0 .. 24"):
        Net((f,), a, d, blocks, [(w, b, 25 if i == 0 else s) for i, (w, b, s) in enumerate(layers)], sp, sv)


def test_sanitized_program(tmp_path):
    """The harness as a program of its own under the host sanitizers."""
    out = str(tmp_path / "pgx_net_main")
    subprocess.run(FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DPGX_NET_MAIN", SRC,
                            "-o", out], check=True)
    run = subprocess.run([out], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert run.stdout.count("mode") == 2


def test_abi_names():
    header = open(os.path.join(ROOT, "include", "envpool_amd.h")).read()
    for name in ("epa_net_create", "epa_net_destroy", "epa_net_eval", "epa_net_eval_device", "epa_net_run",
                 "epa_net_run_device"):
        assert name in native.EXPORTED_SYMBOLS and f"int {name}(" in header
    assert native.check_net_advances(None) == 0 and native.check_net_advances(np.int64(3)) == 3
    for bad in (0, -1, True, 1.5):
        with pytest.raises(ValueError, match="net_run: advances"):
            native.check_net_advances(bad)


class _StandIn:
    """A pool that records its calls: a plain session of k rows whose leaves are all pending until simulations + 1
    advances were made."""

    def __init__(self, k, a, simulations):
        self.k, self.a, self.simulations, self.calls, self.made = k, a, simulations, [], 0

    def _leaves(self):
        st = np.full(self.k, 2 if self.made > self.simulations else 0, np.uint8)
        return np.zeros((self.k, 1, 1, 2), np.bool_), np.ones((self.k, self.a), np.bool_), st

    def guided_begin(self, *args):
        self.calls.append(("begin",) + tuple(args[1:]))
        return self._leaves()

    def gumbel_begin(self, *args):
        self.calls.append(("begin",) + tuple(args[2:]))
        return self._leaves()

    def _advance(self, rows, values):
        assert rows.shape == (self.k, self.a) and values.shape == (self.k,)
        self.calls.append(("advance", self.made))
        self.made += 1
        return self._leaves()

    guided_advance = gumbel_advance = _advance

    def net_run(self, net, leaves, advances=None):
        # what the engine does: evaluation + advance until the round is complete
        assert advances is None and len(leaves) == 3
        while self.made <= self.simulations:
            self._advance(np.zeros((self.k, self.a), np.float32), np.zeros(self.k, np.float32))
        return self._leaves(), self.simulations + 1 - 0

    def guided_result(self):
        self.calls.append(("result",))
        return (np.zeros((self.k, self.a), np.int32), np.zeros((self.k, self.a), np.float32),
                np.zeros(self.k, np.int32))

    def gumbel_result(self):
        return self.guided_result() + (np.zeros((self.k, self.a), np.float32),)

    def guided_end(self):
        self.calls.append(("end",))


def test_run_net_makes_the_calls_of_run_callable():
    k, a, s = 3, 7, 5
    net = Net.random((1, 1, 2), a, 32, 0, seed=1)

    def callable_(obs, mask, status):
        return np.zeros((k, a), np.float32), np.zeros(k, np.float32)

    ids = np.arange(k, dtype=np.int32)
    for make in (lambda p: GuidedSearch(p, ids, s, 1.25, None),
                 lambda p: GumbelSearch(p, ids, s, 4, np.zeros((k, a), np.float32), 50.0, 0.1)):
        seen = []
        for evaluate in (callable_, net):
            pool = _StandIn(k, a, s)
            search = make(pool)
            search.run(evaluate)
            assert search.calls == s + 1 and search._pool is None
            seen.append(pool.calls)
        assert seen[0] == seen[1]
        assert [c[0] for c in seen[0]] == ["begin"] + ["advance"] * (s + 1) + ["result", "end"]
