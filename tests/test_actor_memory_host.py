"""Rollout actor with memory, CPU side: envpool_amd/csrc/actor_memory.hip.h built for the host by g++ against the
contract restated in numpy int64 (actor_memory_util), all integers exact: the cell, the relaid weights against the plain
layout, MemoryParse's refusals, and the torch twin's cell and unroll."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import actor_memory_util as mu
import actor_util as au
from envpool_amd.actor import Actor, Net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("actor_memory") / "libactormemoryhost.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "cpu_harness", "actor_memory_host.cpp"), "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.mh_cell.restype = None
    L.mh_cell.argtypes = ([ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] * 2
                          + [ctypes.c_int] + [ctypes.c_void_p] * 5)
    L.mh_image.restype = ctypes.c_size_t
    L.mh_image.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 3
    L.mh_parse.restype = ctypes.c_int
    L.mh_parse.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    return L


def space(f, kind, h=3):
    return dict(features=f, kind=kind, actions=h, low=np.full(h if kind else 0, -1, np.float32),
                high=np.full(h if kind else 0, 1, np.float32), obs_low=np.full(f, -1.0), obs_high=np.full(f, 1.0))


def check(lib, layers, x, h, reset=None):
    (wz, bz, sz), (wn, bn, sn) = layers
    out, state = np.empty_like(h), np.empty_like(h)
    lib.mh_cell(x.shape[1], h.shape[1], vp(wz), vp(bz), sz, vp(wn), vp(bn), sn, len(x), vp(x), vp(h),
                None if reset is None else vp(reset), vp(out), vp(state))
    want = mu.cell(layers, x, h)
    assert np.array_equal(out, want)
    assert np.array_equal(state, want if reset is None else np.where(reset[:, None] != 0, 0, want))
    return want


@pytest.mark.parametrize("f,m,rows", [(3, 32, 1), (19, 64, 70), (512, 512, 33)])
def test_cell_and_image(lib, f, m, rows):
    rng = np.random.default_rng(f)
    layers = Actor.random(space(f, 0), memory=m, seed=1).cell
    x = rng.integers(0, 128, (rows, f)).astype(np.uint8)
    h = rng.integers(0, 128, (rows, m)).astype(np.uint8)
    want = check(lib, layers, x, h)
    assert len(np.unique(want)) > 16 and (want != h).any(), "the cell must neither saturate nor keep its state"
    reset = (rng.integers(0, 3, rows) == 0).astype(np.uint8)
    reset[0] = 1
    check(lib, layers, x, h, reset)
    # the relaid weights [ct][kt][gate][hh][r][16] against the plain layout with h's columns first and zeros behind K
    steps = (f + m + 31) // 32
    image = np.empty(lib.mh_image(f, m, None, None, None), np.int8)
    lib.mh_image(f, m, vp(layers[0][0]), vp(layers[1][0]), vp(image))
    image = image.reshape(m // 32, steps, 2, 2, 32, 16)
    for g, (w, _, _) in enumerate(layers):
        plain = np.concatenate([w[:, f:], w[:, :f], np.zeros((m, 32 * steps - f - m), np.int8)], axis=1)
        assert np.array_equal(image[:, :, g], plain.reshape(m // 32, 32, steps, 2, 16).transpose(0, 2, 3, 1, 4))


@pytest.mark.parametrize("sign_w,sign_b", [(1, 1), (-1, -1), (1, -1), (-1, 1)])
def test_cell_at_the_accumulator_bound(lib, sign_w, sign_b):
    """All weights +-127, x = h = 127, biases at +-2^30, both ends of the shift: int32 equals int64, h' in 0 .. 127."""
    f = m = 512
    x, h = np.full((2, f), 127, np.uint8), np.full((2, m), 127, np.uint8)
    for shift in (0, 24):
        check(lib, tuple((np.full((m, f + m), s * sign_w * 127, np.int8), np.full(m, s * sign_b * 2**30, np.int32), shift)
                         for s in (1, -1)), x, h)


def parse(lib, blob):
    shape = (ctypes.c_int * 7)()
    err = ctypes.create_string_buffer(256)
    ok = lib.mh_parse(vp(blob), blob.nbytes, shape, err, 256)
    return ok, list(shape), err.value.decode()


def test_parse_refusals(lib):
    f, m = 5, 32
    a = Actor.random(space(f, 1), hidden=32, memory=m, seed=3)
    good = a.blob()
    assert parse(lib, good)[:2] == (1, [f, m, a.cell[0][2], a.cell[1][2], m, 3, 1])
    front = good.nbytes - Actor(a.net, 1, np.zeros(m), np.ones(m), a.sigma, a.low, a.high).blob().nbytes
    w0 = 24 + 16 * f                                  # Wz's first byte; its shift lies behind M K weights and M biases
    patches = [(0, "<i4", au.MAGIC, "magic EPAM"), (4, "<i4", 2, "version"), (12, "<i4", 48, "M = 48"),
               (12, "<i4", 544, "M = 544"), (8, "<i4", 513, "F = 513"), (w0, "i1", -128, "-128"),
               (w0 + m * (f + m) + 4 * m, "<i4", 25, "shift")]
    cases = []
    for at, dtype, value, word in patches:
        bad = good.copy()
        bad[at:at + np.dtype(dtype).itemsize] = np.array([value], dtype).view(np.uint8)
        cases.append((bad, word))
    masked = Actor(Net.random((m,), 3, 32, 1), 2, np.zeros(m), np.ones(m), nvec=[3]).blob()
    cases += [(np.concatenate([good[:front], Actor.random(space(64, 1), hidden=32).blob()]), "must be M"),
              (np.concatenate([good[:front], masked]), "masked"),
              (good[:-4], "bytes"), (np.concatenate([good, np.zeros(4, np.uint8)]), "bytes")]
    for bad, word in cases:
        ok, _, err = parse(lib, bad)
        assert ok == 0 and word in err, (err, word)


@pytest.mark.parametrize("kind", [0, 1])
def test_python_actor_and_torch_twin(lib, tmp_path, kind):
    torch = pytest.importorskip("torch")
    f, m, rows = 19, 64, 9
    a = Actor.random(space(f, kind), hidden=32, memory=m, seed=4)
    assert (a.memory, a.features, a.net.inputs) == (m, f, m) and Actor.random(space(f, kind)).memory == 0
    assert parse(lib, a.blob())[:2] == (1, [f, m, a.cell[0][2], a.cell[1][2], m, 3, kind])
    a.save(str(tmp_path / "a"))
    assert np.array_equal(Actor.load(str(tmp_path / "a")).blob(), a.blob())
    rng = np.random.default_rng(kind)
    obs = rng.uniform(-1.2, 1.2, (4, rows, f))
    h0 = rng.integers(0, 128, (rows, m)).astype(np.uint8)
    mask = rng.integers(0, 2, (4, rows)).astype(bool)
    h, mod = h0, a.module()
    assert np.array_equal(Actor.from_module(mod).blob(), a.blob())
    feat = a.features_of([obs[0]])
    got = mod.cell(torch.tensor(feat, dtype=torch.float64), torch.tensor(h0))
    assert np.array_equal(got.detach().numpy(), mu.cell(a.cell, feat, h0).astype(np.float64))
    logits, value, h_end = mod.unroll(torch.tensor(obs), torch.tensor(h0), torch.tensor(mask))
    assert torch.equal(mod.value(torch.tensor(obs[0]), torch.tensor(h0)), value[0])  # h= reaches forward
    for t in range(4):  # the numpy loop under the state rule
        h = mu.cell(a.cell, a.features_of([obs[t]]), h)
        p = au.head(a.net.layers, a.net.blocks, h)
        assert np.array_equal(logits[t].detach().numpy(), p[:, :3].astype(np.float32) * np.float32(a.net.scale_p))
        assert np.array_equal(value[t].detach().numpy(), p[:, 3].astype(np.float32) * np.float32(a.net.scale_v))
        h = np.where(mask[t][:, None], h, 0).astype(np.uint8)
    assert np.array_equal(h_end.detach().numpy(), h.astype(np.float64))
    logits.sum().backward()
    assert float(mod.cell_weights[0].grad.abs().sum()) > 0
    for refused in (a.trainer, lambda: a.module(kernels=True)):
        with pytest.raises(ValueError, match="memory actor"):
            refused()
