"""Snapshots, CPU side: the index arithmetic of the generator / stack kernels, the blob's size arithmetic and every
header rejection rule (envpool_amd/csrc/snapshot.hip.h built for the host by g++), and the argument checks the Python
layers make before any native call."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from envpool_amd.core import native
from envpool_amd.core.binding import _ShardedPools
from envpool_amd.core.device_pool import DevicePool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MT_WORDS = 624


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("snapshot") / "libsnapshothost.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "cpu_harness", "snapshot_host.cpp"), "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.snap_mt_word_index.restype = ctypes.c_uint64
    L.snap_fnv1a.restype = ctypes.c_uint64
    L.snap_make_header.restype = ctypes.c_uint64
    L.snap_check_header.restype = ctypes.c_char_p
    return L


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def id_lists(n):
    """The whole pool in order, reversed, and the scattered subset of the GPU tests (its ids that exist in a pool
    of n envs, each once: a restore's targets must not repeat)."""
    scattered = []
    for e in [n - 1, 0, 17, 16, 15, 3]:
        if e < n and e not in scattered:
            scattered.append(e)
    return [list(range(n)), list(range(n))[::-1], scattered]


# ---- generator section -----------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 40, 65])
@pytest.mark.parametrize("shift", [0, 4])
def test_generator_pack_then_unpack_is_the_identity(lib, n, shift):
    """Pool image of distinct words -> blob -> a zeroed pool image: the listed columns come back word for word,
    every blob word is written exactly once, no index leaves its section (the harness returns a code otherwise), and
    the blob is laid out like the generator of a pool of k envs."""
    tiled = 1 if shift == 4 else 0
    pool = np.arange(1, MT_WORDS * n + 1, dtype=np.uint32)
    for ids in id_lists(n):
        k = len(ids)
        ids_a = np.asarray(ids, np.int32)
        blob = np.zeros(MT_WORDS * k, np.uint32)
        src = pool.copy()
        assert lib.snap_mt_pass(tiled, 0, _ptr(src), n, shift, _ptr(ids_a), k, _ptr(blob), shift, None, None) == 0
        assert np.array_equal(src, pool)  # packing reads the pool only
        # the blob is the generator of a k-env pool whose env i is env ids[i]
        for i, e in enumerate(ids):
            for j in (0, 1, 15, 16, 17, 226, 227, 396, 397, 623):
                assert blob[lib.snap_mt_word_index(j, i, k, shift)] == pool[lib.snap_mt_word_index(j, e, n, shift)]
        back = np.zeros_like(pool)
        assert lib.snap_mt_pass(tiled, 1, _ptr(back), n, shift, _ptr(ids_a), k, _ptr(blob), shift, None, None) == 0
        cols = np.zeros(n, bool)
        cols[ids] = True
        want = np.zeros_like(pool)
        for e in np.flatnonzero(cols):
            for j in range(MT_WORDS):
                w = lib.snap_mt_word_index(j, int(e), n, shift)
                want[w] = pool[w]
        assert np.array_equal(back, want)  # the listed envs restored, every other word untouched


# A plain restatement of Mt19937 (envpool_amd/csrc/device_common.hip.h): the seeding of InitCommonKernel and the two
# lazy Next() rules, one generator = 624 words in word order + the position of the next word.
MASK32 = 0xFFFFFFFF


def mt_seeded(seed):
    w = np.empty(MT_WORDS, np.uint32)
    x = seed & MASK32
    w[0] = x
    for i in range(1, MT_WORDS):
        x = (1812433253 * (x ^ (x >> 30)) + i) & MASK32
        w[i] = x
    return w


def mt_twist1(cur, nxt, partner):
    y = (cur & 0x80000000) | (nxt & 0x7FFFFFFF)
    return partner ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)


def mt_partner(j):
    return j - 227 if j >= 227 else j + 397


class MtModel:
    """shift 0: word i is twisted when it is consumed; shift 4: the 16 words of a tile when its first word is."""

    def __init__(self, words, pos, shift):
        self.w, self.pos, self.shift = [int(x) for x in words], int(pos), shift

    def _twist(self, j):
        w = self.w
        w[j] = mt_twist1(w[j], w[0 if j == MT_WORDS - 1 else j + 1], w[mt_partner(j)])

    def next(self):
        i = self.pos
        if self.shift == 0:
            self._twist(i)
        elif i % 16 == 0:
            for j in range(i, i + 16):
                self._twist(j)
        y = self.w[i]
        self.pos = 0 if i == MT_WORDS - 1 else i + 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9D2C5680
        y ^= (y << 15) & 0xEFC60000
        y ^= y >> 18
        return y

    def words(self):
        return np.array(self.w, np.uint32)


def numpy_draws(seed, count):
    """The first `count` 32-bit outputs of std::mt19937(seed): numpy's RandomState seeds and tempers alike."""
    return np.random.RandomState(seed).randint(0, 2**32, count, dtype=np.uint64).astype(np.uint32)


def test_the_restated_generators_are_mt19937():
    for shift in (0, 4):
        g = MtModel(mt_seeded(5), 0, shift)
        assert np.array_equal(np.array([g.next() for _ in range(3000)], np.uint32), numpy_draws(5, 3000))


# draws made before the snapshot: the position is draws % 624.  Tile starts, their neighbours, the tiles around the
# partner boundary (word 227) and the last tile (whose word 623 has the regenerated word 0 as its neighbour), and the
# same after one and after three wraps.
MIXED_DRAWS = ([0, 1, 15, 16, 17] + list(range(223, 241)) + list(range(607, 624))
               + [624 + d for d in (0, 1, 5, 15, 16, 229, 600, 623)] + [3 * 624 + d for d in (0, 8, 226, 227, 376, 623)])
MIXED_AFTER = 700


@pytest.fixture(scope="module")
def mixed_pools():
    """Per layout: the generators of a pool whose env e was seeded with 100 + e and has made MIXED_DRAWS[e] draws,
    as (words [n][624] in word order, positions [n])."""
    out = {}
    for shift in (0, 4):
        words, pos = [], []
        for e, draws in enumerate(MIXED_DRAWS):
            g = MtModel(mt_seeded(100 + e), 0, shift)
            for _ in range(draws):
                g.next()
            words.append(g.words())
            pos.append(g.pos)
        out[shift] = (np.stack(words), np.array(pos, np.int32))
    return out


def pool_image(lib, words, shift):
    """[n][624] words in word order -> the flat pool image of that layout."""
    n = words.shape[0]
    img = np.zeros(MT_WORDS * n, np.uint32)
    for e in range(n):
        for j in range(MT_WORDS):
            img[lib.snap_mt_word_index(j, e, n, shift)] = words[e, j]
    return img


def pool_words(lib, img, n, shift):
    idx = np.array([[lib.snap_mt_word_index(j, e, n, shift) for j in range(MT_WORDS)] for e in range(n)])
    return img[idx]


def move_through_a_blob(lib, src_img, src_mti, n, blob_shift, pool_shift, ids, dst_img, dst_mti):
    """Snapshot (the source pool's layout) and restore into a pool image of `pool_shift`, as the engine picks the
    kernels: the tile mapping when both sides are tiled, the word mapping otherwise."""
    k = len(ids)
    ids_a = np.asarray(ids, np.int32)
    blob, blob_mti = np.zeros(MT_WORDS * k, np.uint32), np.zeros(k, np.int32)
    assert lib.snap_mt_pass(1 if blob_shift == 4 else 0, 0, _ptr(src_img), n, blob_shift, _ptr(ids_a), k, _ptr(blob),
                            blob_shift, _ptr(src_mti), _ptr(blob_mti)) == 0
    assert np.array_equal(blob_mti, src_mti[ids_a])
    assert lib.snap_mt_pass(1 if blob_shift == pool_shift == 4 else 0, 1, _ptr(dst_img), n, pool_shift, _ptr(ids_a), k,
                            _ptr(blob), blob_shift, _ptr(dst_mti), _ptr(blob_mti)) == 0


@pytest.mark.parametrize("pool_shift,blob_shift", [(0, 4), (4, 0), (0, 0), (4, 4)])
def test_generator_continues_in_the_other_layout(lib, mixed_pools, pool_shift, blob_shift):
    """A generator restored into a pool of the other layout holds, word for word, what a generator of THAT layout
    holds at the same position, and its next 700 outputs are std::mt19937's.  (Same-layout restores ride along: they
    are plain copies and must stay so.)"""
    n = len(MIXED_DRAWS)
    src_words, src_mti = mixed_pools[blob_shift]
    want_words, want_mti = mixed_pools[pool_shift]
    assert any(p % 16 for p in src_mti) and 0 in src_mti and 623 in src_mti
    src = pool_image(lib, src_words, blob_shift)
    dst, dst_mti = np.zeros(MT_WORDS * n, np.uint32), np.full(n, -1, np.int32)
    move_through_a_blob(lib, src, src_mti.copy(), n, blob_shift, pool_shift, list(range(n))[::-1], dst, dst_mti)
    assert np.array_equal(dst_mti, want_mti)
    got = pool_words(lib, dst, n, pool_shift)
    bad = np.argwhere(got != want_words)
    assert bad.size == 0, [(MIXED_DRAWS[e], j) for e, j in bad[:8]]
    for e, draws in enumerate(MIXED_DRAWS):
        g = MtModel(got[e], dst_mti[e], pool_shift)
        out = np.array([g.next() for _ in range(MIXED_AFTER)], np.uint32)
        assert np.array_equal(out, numpy_draws(100 + e, draws + MIXED_AFTER)[draws:]), draws


@pytest.mark.parametrize("pool_shift,blob_shift", [(0, 4), (4, 0)])
def test_generator_moves_between_layouts(lib, pool_shift, blob_shift):
    """A blob restored into a pool built with the other generator layout: the word mapping moves every word outside
    the tile that holds the position verbatim -- and all words of an env whose position starts a tile -- into the
    listed columns only, and the positions with them.  The words of the partly consumed tile in front of the
    position stay too (they are the new block's in both layouts); what the rest of that tile becomes is
    test_generator_continues_in_the_other_layout's subject."""
    n, ids = 40, [39, 0, 17, 16, 15, 3]
    k = len(ids)
    src = np.arange(1, MT_WORDS * n + 1, dtype=np.uint32)  # in the blob's layout
    src_mti = ((np.arange(n) * 37 + 6) % MT_WORDS).astype(np.int32)
    src_mti[[0, 16]] = [0, 608]  # two of the listed envs are at a tile start
    assert sum(src_mti[e] % 16 != 0 for e in ids) == k - 2
    dst, dst_mti = np.zeros(MT_WORDS * n, np.uint32), np.full(n, -1, np.int32)
    move_through_a_blob(lib, src, src_mti.copy(), n, blob_shift, pool_shift, ids, dst, dst_mti)
    touched = np.zeros(MT_WORDS * n, bool)
    for e in ids:
        p = int(src_mti[e])
        assert dst_mti[e] == p
        for j in range(MT_WORDS):
            w = lib.snap_mt_word_index(j, e, n, pool_shift)
            touched[w] = True
            if p % 16 == 0 or not p <= j <= (p | 15):
                assert dst[w] == src[lib.snap_mt_word_index(j, e, n, blob_shift)], (e, j)
    assert not dst[~touched].any()  # no other env's word is written
    others = np.setdiff1d(np.arange(n), ids)
    assert (dst_mti[others] == -1).all()


def test_word_index_is_the_step_kernels_layout(lib):
    """MtWordIndex against the formula of Mt19937::At written out: [624][N] and [39][N][16]."""
    n = 40
    for e in (0, 17, 39):
        for j in (0, 15, 16, 623):
            assert lib.snap_mt_word_index(j, e, n, 0) == j * n + e
            assert lib.snap_mt_word_index(j, e, n, 4) == ((j // 16) * n + e) * 16 + j % 16


# ---- stack section ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 40, 65])
@pytest.mark.parametrize("length", [51, 54, 1])  # 3 x 17 (odd: the narrow kernel), 2 x 27 (pairs), one double
def test_stack_pack_then_unpack_is_the_identity(lib, n, length):
    ring = np.arange(1, n * length + 1, dtype=np.float64)
    for ids in id_lists(n):
        k = len(ids)
        ids_a = np.asarray(ids, np.int32)
        blob = np.zeros(k * length)
        assert lib.snap_stack_pass(0, _ptr(ring), n, _ptr(ids_a), k, length, _ptr(blob)) == 0
        assert np.array_equal(blob.reshape(k, length), ring.reshape(n, length)[ids])
        back = np.zeros_like(ring)
        assert lib.snap_stack_pass(1, _ptr(back), n, _ptr(ids_a), k, length, _ptr(blob)) == 0
        want = np.zeros((n, length))
        want[ids] = ring.reshape(n, length)[ids]
        assert np.array_equal(back.reshape(n, length), want)


# ---- header ----------------------------------------------------------------------------------
def desc(family="HalfCheetah", num_envs=40, state_dim=34, has_rng=1, mt_shift=0, stack_s=1, stack_nobs=0, extra=0,
         lib=None):
    return (ctypes.c_uint64 * 8)(lib.snap_fnv1a(family.encode()), num_envs, state_dim, has_rng, mt_shift, stack_s,
                                 stack_nobs, extra)


def header(lib, d, k, flags=1):
    buf = np.zeros(64, np.uint8)
    total = lib.snap_make_header(d, k, flags, _ptr(buf))
    return buf, total


def up64(x):
    return (x + 63) // 64 * 64


def test_fnv1a_of_the_family_name(lib):
    assert lib.snap_fnv1a(b"") == 0xCBF29CE484222325
    assert lib.snap_fnv1a(b"a") == 0xAF63DC4C8601EC8C
    assert lib.snap_fnv1a(b"Hex") != lib.snap_fnv1a(b"Othello")


@pytest.mark.parametrize("k", [1, 6, 40])
@pytest.mark.parametrize("flags,has_rng", [(1, 1), (0, 1), (1, 0)])
@pytest.mark.parametrize("stack", [(1, 0), (3, 17)])
def test_snapshot_bytes_arithmetic(lib, k, flags, has_rng, stack):
    """The byte count written out: 64 header bytes, then every section rounded up to 64 bytes; the generator
    section only with the flag AND a pool that has generators, the stack section only with frame_stack > 1."""
    s, nobs = stack
    dim = 34
    d = desc(lib=lib, has_rng=has_rng, mt_shift=4, stack_s=s, stack_nobs=nobs)
    buf, total = header(lib, d, k, flags)
    rng = bool(flags and has_rng)
    want = 64 + up64(8 * k * dim)
    off_mt = want
    if rng:
        want = up64(want + 4 * 624 * k + 4 * k)
    off_stack = want
    if s > 1:
        want = up64(want + 8 * k * s * nobs + 4 * k)
    assert total == want
    lay = (ctypes.c_uint64 * 7)()
    lib.snap_layout(_ptr(buf), lay)
    assert lay[0] == 64 and lay[1] == off_mt and lay[3] == off_stack and lay[6] == total
    assert lay[2] == off_mt + (4 * 624 * k if rng else 0) and lay[4] == off_stack + (8 * k * s * nobs if s > 1 else 0)
    assert all(int(o) % 64 == 0 for o in (lay[0], lay[1], lay[3], lay[5], lay[6]))
    # the fields the Python side reads
    assert int(buf[20:24].view("<i4")[0]) == k and int(buf[48:56].view("<u8")[0]) == total
    assert int(buf[24:28].view("<u4")[0]) == (1 if rng else 0)
    assert lib.snap_check_header(d, _ptr(buf), k) is None
    if rng:
        _, without = header(lib, d, k, 0)
        assert total - without == up64(4 * 624 * k + 4 * k)  # shorter by the generator section


def test_every_header_rejection_rule(lib):
    d = desc(lib=lib, mt_shift=4, stack_s=3, stack_nobs=17)
    good, total = header(lib, d, 6)
    assert lib.snap_check_header(d, _ptr(good), 6) is None

    def refused(pool_desc, buf, k=6):
        msg = lib.snap_check_header(pool_desc, _ptr(buf), k)
        assert msg is not None
        return msg.decode()

    def patched(offset, fmt, value):
        b = good.copy()
        b[offset:offset + np.dtype(fmt).itemsize].view(fmt)[0] = value
        return b

    assert "magic" in refused(d, patched(0, "<u4", 0x12345678))
    assert "version" in refused(d, patched(4, "<u4", 2))
    assert "family" in refused(desc("Ant", lib=lib, mt_shift=4, stack_s=3, stack_nobs=17), good)
    assert "state_dim" in refused(desc(lib=lib, state_dim=35, mt_shift=4, stack_s=3, stack_nobs=17), good)
    assert "frame_stack" in refused(desc(lib=lib, mt_shift=4), good)                            # stacked blob, plain pool
    assert "frame_stack" in refused(desc(lib=lib, mt_shift=4, stack_s=3, stack_nobs=18), good)  # another nobs
    assert "frame_stack" in refused(desc(lib=lib, mt_shift=4, stack_s=2, stack_nobs=17), good)  # another depth
    assert "generators" in refused(desc(lib=lib, has_rng=0, stack_s=3, stack_nobs=17), good)
    assert "flags" in refused(d, patched(24, "<u4", 3))
    assert "generator layout" in refused(d, patched(28, "<i4", 2))
    assert "family section" in refused(d, patched(40, "<u8", 8))
    assert "env count" in refused(d, patched(20, "<i4", 0))
    assert "env count" in refused(d, patched(20, "<i4", 41), k=41)
    assert "another number of envs" in refused(d, good, k=5)
    assert "byte count" in refused(d, patched(48, "<u8", total - 64))
    assert "byte count" in refused(d, patched(48, "<u8", total + 64))
    # a blob without generators fits a pool with them (its generators are left alone), in either layout
    plain, _ = header(lib, d, 6, 0)
    assert lib.snap_check_header(d, _ptr(plain), 6) is None
    assert lib.snap_check_header(desc(lib=lib, mt_shift=0, stack_s=3, stack_nobs=17), _ptr(good), 6) is None
    plain[28:32].view("<i4")[0] = 4  # ... but names no layout
    assert "generator layout" in refused(d, plain)


# ---- Python argument checks ------------------------------------------------------------------
class _NoNative:
    """Stands in for the C library: any call is a test failure."""

    def __getattr__(self, name):
        raise AssertionError(f"native call {name} reached")


def fake_device_pool(num_envs=40, offset=0):
    p = object.__new__(DevicePool)
    p._lib, p._h = _NoNative(), None
    p.num_envs, p.env_id_offset = num_envs, offset
    return p


def test_short_blob_raises_before_any_native_call(lib):
    pool = fake_device_pool()
    with pytest.raises(ValueError, match="shorter than a header"):
        pool.restore(np.zeros(10, np.uint8))
    blob, total = header(lib, desc(lib=lib), 6)
    with pytest.raises(ValueError, match="shorter than its header says"):
        pool.restore(np.concatenate([blob, np.zeros(total - 64 - 1, np.uint8)]))
    with pytest.raises(ValueError, match="uint8"):
        pool.restore(np.zeros(128, np.float64))
    assert native.snapshot_header(np.concatenate([blob, np.zeros(total - 64, np.uint8)])) == (6, total)


class _Recorder:
    def __init__(self, offset, per):
        self.env_id_offset, self.num_envs, self.calls = offset, per, []

    def snapshot(self, env_ids, rng):
        self.calls.append(("snapshot", env_ids, rng))
        return np.zeros(64, np.uint8)

    def restore(self, blob, env_ids):
        self.calls.append(("restore", env_ids))

    def fork(self, src, dst, rng):
        self.calls.append(("fork", list(src), list(dst), rng))


@pytest.fixture()
def sharded():
    import concurrent.futures

    s = object.__new__(_ShardedPools)
    s.per, s.offset = 20, 100
    s.pools = [_Recorder(100, 20), _Recorder(120, 20)]
    s._exec = concurrent.futures.ThreadPoolExecutor(2)
    yield s
    s._exec.shutdown(wait=True)


def test_sharded_snapshot_and_restore_take_no_env_ids(sharded, lib):
    with pytest.raises(ValueError, match="env_ids"):
        sharded.snapshot([100, 101])
    with pytest.raises(ValueError, match="env_ids"):
        sharded.restore([None, None], env_ids=[100])
    with pytest.raises(ValueError, match="list of 2 blobs"):
        sharded.restore(np.zeros(64, np.uint8))
    assert not sharded.pools[0].calls and not sharded.pools[1].calls
    blobs = sharded.snapshot()
    assert len(blobs) == 2 and [p.calls for p in sharded.pools] == [[("snapshot", None, True)]] * 2
    shard_blob, total = header(lib, desc(lib=lib), 20)
    full = np.concatenate([shard_blob, np.zeros(total - 64, np.uint8)])
    sharded.restore([full, full])
    assert [p.calls[-1] for p in sharded.pools] == [("restore", None)] * 2
    other, total6 = header(lib, desc(lib=lib), 6)
    with pytest.raises(ValueError, match="20 envs of its shard"):
        sharded.restore([full, np.concatenate([other, np.zeros(total6 - 64, np.uint8)])])


def test_sharded_fork_stays_inside_a_shard(sharded):
    with pytest.raises(ValueError, match="across shards"):
        sharded.fork([100, 101], [102, 120])
    with pytest.raises(ValueError, match="out of range"):
        sharded.fork([100], [140])
    with pytest.raises(ValueError, match="source ids"):
        sharded.fork([100, 101], [102])
    assert not sharded.pools[0].calls and not sharded.pools[1].calls
    sharded.fork([100, 121, 100], [105, 139, 106], rng=False)
    assert sharded.pools[0].calls == [("fork", [100, 100], [105, 106], False)]
    assert sharded.pools[1].calls == [("fork", [121], [139], False)]


def test_env_mixin_forwards_global_ids():
    """env.snapshot / restore / fork of a gymnasium pool: ids normalised to int32 arrays, None kept."""
    from envpool_amd.pgx import OthelloGymnasiumEnvPool

    env = object.__new__(OthelloGymnasiumEnvPool)
    env._pool = _Recorder(0, 40)
    env.snapshot()
    env.snapshot(3, rng=False)
    env.restore(np.zeros(64, np.uint8), [1, 2])
    env.fork([3, 3], [10, 11])
    calls = env._pool.calls
    assert calls[0] == ("snapshot", None, True)
    assert calls[1][0] == "snapshot" and calls[1][1].dtype == np.int32 and list(calls[1][1]) == [3] and not calls[1][2]
    assert calls[2][0] == "restore" and list(calls[2][1]) == [1, 2]
    assert calls[3] == ("fork", [3, 3], [10, 11], True)
