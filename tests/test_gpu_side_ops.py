"""get_state / set_state, render and snapshot / restore / fork share one path inside the engine (Pool::SideEnter,
SideIds, SideScratch, SideLeave): the env ids of a call go up through two rotating slots or not at all, host forms
copy through one scratch block per pool, and on an async pool every call is ordered against the steps of all compute
streams.  These tests mix the features on one pool, where a stale id list, a scratch block reused too early or a
missing stream dependency would show; they say nothing about memory footprint.

Every pool has 40 envs: no multiple of 64, and fewer than the 1024 entries an id slot starts with."""
import ctypes

import numpy as np
import pytest

from envpool_amd.core import native
from envpool_amd.core.device_pool import DevicePool

pytestmark = pytest.mark.gpu

N = 40
OFF = 100
BATCH = 8
# (discrete action count or None for a box of that width, max_episode_steps: short, so that a window holds resets)
TASKS = {"CartPole": (2, 7), "HalfCheetah": (None, 7), "Snake": (4, 6)}


def make(family, seed=11, batch_size=0, streams=None, env_id_offset=0):
    params = None if streams is None else {"compute_streams": float(streams)}
    return DevicePool(family, N, batch_size=batch_size, seed=seed, max_episode_steps=TASKS[family][1],
                      env_id_offset=env_id_offset, params=params)


def actions(pool, rng, k):
    n = TASKS[pool.family][0]
    if n is None:
        return rng.uniform(-1, 1, (k, *pool.action_shape)).astype(pool.action_dtype)
    return rng.integers(0, n, (k, *pool.action_shape)).astype(pool.action_dtype)


def all_ids(pool):
    return np.arange(pool.env_id_offset, pool.env_id_offset + N, dtype=np.int32)


def same(a, b, tag):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (tag, a.shape, b.shape, a.dtype, b.dtype)
    bad = np.argwhere(a.view(np.uint8) != b.view(np.uint8))
    assert bad.size == 0, (tag, bad[:4].tolist())


def free_run(pools, rng, steps, between=None):
    """Async twins: `steps` times one recv of BATCH rows and the send that answers it; 40 - 8 rows stay un-received
    throughout.  The twins must return the same rows in every key; `between(t)` runs after each send."""
    for t in range(steps):
        outs = [p.recv_dict() for p in pools]
        for key in outs[0]:
            same(outs[0][key], outs[1][key], (t, key))
        ids = outs[0]["info:env_id"]
        assert ids.shape == (BATCH,)
        act = actions(pools[0], rng, BATCH)
        for p in pools:
            p.send(ids, act)
        if between is not None:
            between(t)


def warmed(family, steps=9, **kw):
    """A sync pool after `steps` seeded whole-pool steps: its envs have gone their own ways."""
    pool = make(family, **kw)
    ids, rng = all_ids(pool), np.random.default_rng(21)
    pool.reset(ids)
    pool.recv()
    for _ in range(steps):
        pool.send(ids, actions(pool, rng, N))
        pool.recv()
    return pool


def snap_rows(blob):
    """The envs of a snapshot blob one by one: [k, bytes].  The layout is DEFINED in envpool_amd/csrc/snapshot.hip.h
    (its head comment, `struct Header`, `LayoutOf`): state [k][dim], generator words [624][k] or [39][k][16], their
    positions [k], every section on a 64-byte boundary; pools here have neither a frame stack nor an extra section.
    A change of the blob format has to be followed here (the asserts below catch a version they do not understand)."""
    assert int(blob[:8].view("<u4")[1]) == 1, "snapshot.hip.h: kVersion has changed, and with it maybe the layout"
    head = blob[:64]
    dim, k, flags, shift, stack_s = (int(x) for x in head[16:36].view("<i4"))
    assert stack_s == 1 and int(head[40:48].view("<u8")[0]) == 0 and int(head[48:56].view("<u8")[0]) == blob.nbytes
    up = lambda x: (x + 63) // 64 * 64
    parts = [blob[64:64 + 8 * k * dim].reshape(k, -1)]
    off = up(64 + 8 * k * dim)
    if flags & 1:
        words = blob[off:off + 4 * 624 * k].view("<u4")
        words = words.reshape(39, k, 16).transpose(1, 0, 2) if shift == 4 else words.reshape(624, k).T
        parts.append(np.ascontiguousarray(words).reshape(k, -1).view(np.uint8))
        off += 4 * 624 * k
        parts.append(blob[off:off + 4 * k].reshape(k, -1))
        off = up(off + 4 * k)
    assert off == blob.nbytes
    return np.concatenate(parts, axis=1)


@pytest.mark.parametrize("streams", [1, 4])
@pytest.mark.parametrize("family", ["CartPole", "HalfCheetah"])
def test_state_amid_an_async_rollout_with_an_id_offset(family, streams):
    a, b = (make(family, batch_size=BATCH, streams=streams, env_id_offset=OFF) for _ in range(2))
    rng = np.random.default_rng(5)
    for p in (a, b):
        p.reset(all_ids(p))
    free_run((a, b), rng, 12)
    ids = OFF + np.array([39, 0, 17, 16, 15, 3, 17, 22], dtype=np.int32)  # permuted, 17 twice
    rows = a.get_state(ids)
    same(rows[2], rows[6], "the duplicate")
    a.set_state(rows, ids)
    same(a.get_state(ids), rows, "read back")
    free_run((a, b), rng, 6)
    same(a.get_state(), b.get_state(), "whole pool, at the end")
    same(a.get_state()[ids - OFF], a.get_state(ids), "rows of the whole-pool call")
    a.close(), b.close()


def test_id_slot_rotation_and_the_in_order_shortcut():
    pool = warmed("Snake", env_id_offset=OFF)
    state, frames, blob = pool.get_state(), pool.render(all_ids(pool)), snap_rows(pool.snapshot())
    assert len({s.tobytes() for s in state}) > N // 2
    k = 7
    lists = [np.array(x, dtype=np.int32) for x in
             ([39, 0, 17, 16, 15, 3, 38], [1, 38, 5, 20, 21, 9, 2], [33, 32, 31, 4, 19, 18, 0])]
    lists += [np.arange(k, dtype=np.int32), np.arange(N, dtype=np.int32)]
    # every feature meets every list; the calls of one round alternate between the features
    for shift in range(3):
        for i, loc in enumerate(lists):
            what = (i + shift) % 3
            if what == 0:
                same(pool.get_state(loc + OFF), state[loc], ("get_state", shift, i))
            elif what == 1:
                same(pool.render(loc + OFF), frames[loc], ("render", shift, i))
            else:
                same(snap_rows(pool.snapshot(loc + OFF)), blob[loc], ("snapshot", shift, i))
    pool.close()


def test_scratch_is_shared_across_features_and_grows():
    pool = warmed("Snake")
    many = np.arange(100, dtype=np.int32) * 7 % N  # 100 rows of a 40-env pool
    src, dst = np.array([3, 3, 39, 0], dtype=np.int32), np.array([10, 0, 11, 25], dtype=np.int32)
    calls = [lambda p: p.snapshot([5]), lambda p: p.render(many), lambda p: p.get_state(),
             lambda p: (p.fork(src, dst), p.get_state(dst))[1]]
    got = [call(pool) for call in calls]
    assert got[0].nbytes < got[1].nbytes > got[2].nbytes  # the block has to grow, then a smaller user follows
    for i, call in enumerate(calls):
        twin = warmed("Snake")
        same(got[i], call(twin), ("call", i))
        twin.close()
    same(got[3], got[2][src], "forked rows")
    pool.close()


def test_device_forms_on_an_async_pool():
    torch = pytest.importorskip("torch")
    from envpool_amd import torch_interop as ti

    a, b = (make("Snake", batch_size=BATCH, streams=4) for _ in range(2))
    rng = np.random.default_rng(6)
    for p in (a, b):
        p.reset(all_ids(p))
    free_run((a, b), rng, 12)
    ids = np.array([39, 0, 17, 16, 15, 3, 17, 22], dtype=np.int32)
    uniq = np.array([1, 38, 5, 20, 21, 9], dtype=np.int32)
    frames = ti.render_device(a, ids)
    blob = ti.snapshot_device(a, uniq)
    ti.restore_device(a, blob, uniq)
    frames2 = ti.render_device(a, ids, 16, 16)
    assert frames.dtype == torch.uint8 and frames.is_cuda and blob.is_cuda
    same(frames.cpu().numpy(), a.render(ids), "frames")
    same(frames2.cpu().numpy(), a.render(ids, 16, 16), "frames after the restore")
    same(blob.cpu().numpy(), a.snapshot(uniq), "blob")

    def between(t):  # ... and with steps in flight on every stream
        ti.restore_device(a, ti.snapshot_device(a, uniq), uniq)
        ti.render_device(a, ids, 16, 16)

    free_run((a, b), rng, 6, between)
    same(a.get_state(), b.get_state(), "whole pool, at the end")
    a.close(), b.close()


@pytest.mark.parametrize("batch_size", [0, BATCH])
def test_refusals_leave_the_pool_usable(batch_size):
    pool, cart = make("Snake", batch_size=batch_size), make("CartPole", batch_size=batch_size)
    lib = native.lib()
    for p in (pool, cart):
        p.reset(all_ids(p))
        p.recv()
    ids = np.array([39, 0, 17, 17], dtype=np.int32)
    want = {p: p.get_state(ids) for p in (pool, cart)}
    dim = pool.state_dim()
    buf = np.zeros((N + 1) * dim, dtype=np.float64)
    too_many = np.zeros(N + 1, dtype=np.int32)
    blob = pool.snapshot(ids[:3])
    spare = ctypes.create_string_buffer(blob.nbytes + 16)  # (host memory, never dereferenced: the pool refuses first)
    aligned = (ctypes.addressof(spare) + 15) // 16 * 16
    w, h = pool.render_size()
    rgb = np.zeros((N + 1) * h * w * 3, dtype=np.uint8)
    p_ids, p_buf, p_rgb, p_blob = ids.ctypes.data, buf.ctypes.data, rgb.ctypes.data, blob.ctypes.data
    R, V = RuntimeError, ValueError
    refused = [
        (pool, V, "get_state: null argument", lambda: lib.epa_get_state(pool._h, None, 4, p_buf)),
        (pool, V, "get_state: null argument", lambda: lib.epa_get_state(pool._h, p_ids, 4, None)),
        (pool, V, "set_state: null argument", lambda: lib.epa_set_state(pool._h, None, 4, p_buf)),
        (pool, V, "set_state: null argument", lambda: lib.epa_set_state(pool._h, p_ids, 4, None)),
        (pool, V, f"batch of {N + 1} rows exceeds num_envs", lambda: pool.get_state(too_many + N)),  # (the count first)
        (pool, V, f"batch of {N + 1} rows exceeds num_envs", lambda: pool.set_state(buf.reshape(N + 1, dim), too_many)),
        (pool, V, f"env_id {N} out of range", lambda: pool.get_state([0, N])),
        (pool, V, "env_id -1 out of range", lambda: pool.set_state(buf[:2 * dim].reshape(2, dim), [0, -1])),
        (pool, V, "render: null argument", lambda: lib.epa_render(pool._h, None, 4, 0, 0, -1, p_rgb)),
        (pool, V, "render: null argument", lambda: lib.epa_render(pool._h, p_ids, 4, 0, 0, -1, None)),
        (pool, V, "render: null argument", lambda: lib.epa_render_device(pool._h, p_ids, 4, 0, 0, -1, None)),
        (pool, V, "render env_ids must not be empty", lambda: lib.epa_render(pool._h, p_ids, 0, 0, 0, -1, p_rgb)),
        (pool, V, f"env_id {N} out of range", lambda: pool.render([0] * N + [N])),  # (any count: the ids alone)
        # a family that does not render says so whatever the ids
        (cart, R, "render not implemented for this environment",
         lambda: lib.epa_render(cart._h, (too_many + N).ctypes.data, N + 1, 0, 0, -1, p_rgb)),
        (cart, R, "render not implemented for this environment", lambda: lib.epa_render(cart._h, None, 0, 0, 0, -1, None)),
        (pool, V, "snapshot: null argument", lambda: lib.epa_snapshot(pool._h, None, 3, 1, p_blob, blob.nbytes)),
        (pool, V, "snapshot: null argument", lambda: lib.epa_snapshot(pool._h, p_ids, 3, 1, None, blob.nbytes)),
        (pool, V, "snapshot: null argument", lambda: pool.snapshot_device(0, ids[:3])),
        (pool, V, "snapshot env_ids must not be empty", lambda: lib.epa_snapshot(pool._h, p_ids, 0, 1, p_blob, blob.nbytes)),
        (pool, V, f"batch of {N + 1} rows exceeds num_envs",
         lambda: lib.epa_snapshot(pool._h, too_many.ctypes.data, N + 1, 1, p_blob, blob.nbytes)),
        (pool, V, f"snapshot of {N + 1} envs: must be 1 .. num_envs", lambda: pool.snapshot_bytes(N + 1)),
        (pool, V, f"env_id {N} out of range", lambda: pool.snapshot([N])),
        (pool, V, "snapshot: unknown flags", lambda: lib.epa_snapshot(pool._h, p_ids, 3, 2, p_blob, blob.nbytes)),
        (pool, V, f"snapshot: buffer of 64 bytes, the blob needs {blob.nbytes}",
         lambda: lib.epa_snapshot(pool._h, p_ids, 3, 1, p_blob, 64)),
        (pool, V, "snapshot: the device blob must be 16-byte aligned", lambda: pool.snapshot_device(aligned + 4, ids[:3])),
        (pool, V, "snapshot: env_id 17 is restored into twice", lambda: pool.restore(blob, [0, 17, 17])),
        (pool, V, "snapshot: env_id 17 is restored into twice", lambda: pool.fork([0, 1], [17, 17])),
        (pool, V, "restore: null argument", lambda: lib.epa_restore(pool._h, p_ids, 3, None, blob.nbytes)),
        (pool, V, "restore: null argument", lambda: lib.epa_restore_device(pool._h, p_ids, 3, aligned, None)),
        (pool, V, "snapshot: blob shorter than a header", lambda: lib.epa_restore(pool._h, p_ids, 3, p_blob, 40)),
        (pool, V, "snapshot: blob shorter than its header says",
         lambda: lib.epa_restore(pool._h, p_ids, 3, p_blob, blob.nbytes - 64)),
        (pool, V, "another number of envs", lambda: pool.restore(blob, [0, 1])),
        (cart, V, "another env family", lambda: cart.restore(blob, [0, 1, 2])),
    ]
    for i, (p, exc, text, call) in enumerate(refused):
        with pytest.raises(exc) as err:
            code = call()
            if isinstance(code, int):  # (a raw C ABI call: the wrappers have raised by themselves)
                native.check(code)
        assert text in str(err.value), (i, text, str(err.value))
        same(p.get_state(ids), want[p], ("get_state after refusal", i, text))  # nothing was left half-entered
    pool.set_state(buf[:0].reshape(0, dim), [])  # k == 0: nothing to do
    assert pool.get_state([]).shape == (0, dim)
    pool.close(), cart.close()
