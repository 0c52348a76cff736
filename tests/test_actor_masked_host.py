"""The masked head of the rollout actor (kind 2), CPU side: csrc/actor.hip.h built for the host by g++ against the numpy
restatement (actor_masked_util) bit for bit, ActorParse on kind-2 blobs, `space_of` and `Actor` on the Jumanji specs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import actor_masked_util as mu
import actor_util as au
import envpool_amd as envpool
from envpool_amd import actor as actor_mod
from test_actor_host import head_rows, vp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("actor_masked") / "libactormaskedhost.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "cpu_harness", "actor_masked_host.cpp"), "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.amh_parse.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    L.amh_sample.restype = None
    L.amh_sample.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                             ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int] + \
                            [ctypes.c_void_p] * 5
    return L


def parse(lib, blob):
    shape, err = (ctypes.c_int * 11)(), ctypes.create_string_buffer(256)
    return lib.amh_parse(vp(blob), blob.nbytes, shape, err, 256), list(shape), err.value.decode()


# the int32 words mask0, C, nvec[4] of Game2048's blob (F = 20, H = 4) lie behind lo and scale
@pytest.mark.parametrize("word,at,value", [(None, 0, 16), (None, 0, -1), (None, 0, 0), ("C =", 1, 0), ("C =", 1, 5),
                                           ("product", 2, 2), ("nvec[2]", 4, 2), ("nvec[0]", 2, 0), ("mask0", 0, 17),
                                           ("mask0", 0, -2)])
def test_parse(lib, word, at, value):
    a = actor_mod.Actor.random(envpool.make_spec("Game2048-v1"), hidden=32, seed=3, mask=True)
    blob = a.blob()
    assert parse(lib, blob)[:2] == (1, [20, 4, 32, 1, 2, 16, 1, 4, 1, 1, 1])
    blob[36 + 16 * 20 + 4 * at:][:4] = np.array([value], "<i4").view(np.uint8)
    ok, shape, err = parse(lib, blob)
    assert (ok == 1 and shape[5] == value) if word is None else (ok == 0 and word in err), err
    assert parse(lib, blob[:36 + 16 * 20 + 8])[0] == 0   # (ends inside the masked section)


@pytest.mark.parametrize("h,nvec", [(2, (2,)), (9, (3, 3)), (64, (64,)), (65, (5, 13)), (100, (10, 10)), (127, (127,)),
                                    (24, (2, 3, 4)), (16, (2, 2, 2, 2))])
@pytest.mark.parametrize("deterministic", [False, True])
def test_sample_equals_the_restatement(lib, h, nvec, deterministic):
    rng = np.random.default_rng(h)
    rows, c = 70, len(nvec)
    p, m = head_rows(rng, rows, h), mu.masks(rng, rows, h)
    raw = np.ascontiguousarray(m * rng.integers(1, 200, (rows, h)), np.uint8)   # any value that is not 0 counts
    legal = mu.legal_of(m)
    ids = (np.arange(rows) + 1000).astype(np.int32)
    sp, sv = F32(1 / 4096), F32(1 / 2048)
    nv = np.array(list(nvec) + [1] * (4 - c), np.int32)
    action, logp, value = np.empty((rows, c), np.int32), np.empty(rows, F32), np.empty(rows, F32)
    words = np.empty((rows, 4), np.uint32)
    lib.amh_sample(vp(p), vp(raw), rows, h, sp, sv, 11, vp(ids), 5, int(deterministic), c, vp(nv), vp(action), vp(logp),
                   vp(value), vp(words))
    wa, wl, wv = mu.sample(p, legal, sp, sv, 11, ids, 5, deterministic)
    assert np.array_equal(words, mu.words(m)) and legal[np.arange(rows), wa].all()
    assert np.array_equal(action, np.stack(np.unravel_index(wa, nvec), axis=1))   # mixed radix, most significant first
    assert np.array_equal(logp.view(np.uint32), wl.view(np.uint32)) and np.array_equal(value, wv)
    if deterministic:
        assert np.array_equal(wa, np.where(legal, p[:, :h], -2**31).argmax(axis=1))
    # the rows whose set is everything (2: all legal, 3: none legal) are the discrete head's, bit for bit
    da, dl, _ = au.discrete(p[2:4], sp, sv, 11, ids[2:4], 5, deterministic)
    assert np.array_equal(wa[2:4], da) and np.array_equal(wl[2:4].view(np.uint32), dl.view(np.uint32))


def test_space_of_and_the_python_layers(lib, tmp_path):
    mine = actor_mod.space_of(envpool.make_spec("Minesweeper-v0"))
    assert (mine["kind"], mine["actions"], mine["mask0"], list(mine["nvec"])) == (2, 100, -1, [10, 10])
    g = envpool.make_spec("Game2048-v1")
    assert actor_mod.space_of(g)["kind"] == 0 and "mask0" not in actor_mod.space_of(g)
    for mask in (True, "obs:action_mask"):
        s = actor_mod.space_of(g, mask=mask)
        assert (s["kind"], s["actions"], s["mask0"], list(s["nvec"])) == (2, 4, 16, [4])
    for task, mask in (("Game2048-v1", "obs:board"), ("Game2048-v1", "obs:nothing"), ("Pendulum-v1", True),
                       ("CartPole-v1", True)):
        with pytest.raises(ValueError, match="mask"):
            actor_mod.space_of(envpool.make_spec(task), mask=mask)
    a = actor_mod.Actor.random(envpool.make_spec("Minesweeper-v0"), hidden=32, seed=3, mask=True)
    assert parse(lib, a.blob())[:2] == (1, [202, 100, 32, 1, 2, 100, 2, 10, 10, 1, 1])
    a.save(str(tmp_path / "mine.npz"))
    assert np.array_equal(actor_mod.Actor.load(str(tmp_path / "mine.npz")).blob(), a.blob())
    for bad in (dict(mask0=103, nvec=[10, 10]), dict(mask0=100, nvec=[10, 9])):
        with pytest.raises(ValueError, match="mask0|nvec"):
            actor_mod.Actor(a.net, 2, a.lo, a.scale, **bad)
