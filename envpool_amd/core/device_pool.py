"""`DevicePool`: thin object over the C ABI for one env family.

It plays the role of the C++ `EnvPool<Spec>` virtual interface of the reference
(envpool/core/envpool.h:29-56: Send / Recv / Reset) — the thing
`PyEnvPool` wraps — with the thread pool replaced by batched HIP kernels.
"""

from __future__ import annotations

import collections
import ctypes
import threading
import weakref
from typing import Any, Sequence

import numpy as np

from . import native


class _PinnedBlocks:
    """Free list of pinned host blocks (epa_host_alloc) that back the arrays
    `recv` returns.  A block is lent to ONE batch: the per-key numpy arrays are
    views of it, and it only comes back here when the last of them is garbage
    collected — so, like the reference's capsule-owned buffers
    (py_envpool.h:40-49), an array is never overwritten by a later step."""

    _MAX_FREE = 4  # per size

    def __init__(self, lib: Any) -> None:
        self._lib = lib
        self._free: dict[int, list[int]] = collections.defaultdict(list)
        self._lock = threading.Lock()
        self._closed = False

    def take(self, nbytes: int) -> np.ndarray:
        with self._lock:
            free = self._free[nbytes]
            ptr = free.pop() if free else None
        if ptr is None:
            ptr = self._lib.epa_host_alloc(nbytes)
            if not ptr:
                raise MemoryError(f"epa_host_alloc({nbytes}) failed")
        base = np.ctypeslib.as_array((ctypes.c_ubyte * nbytes).from_address(ptr))
        fin = weakref.finalize(base, self._give_back, nbytes, ptr)
        fin.atexit = False  # process teardown frees pinned memory anyway
        return base

    def _give_back(self, nbytes: int, ptr: int) -> None:
        with self._lock:
            if not self._closed and len(self._free[nbytes]) < self._MAX_FREE:
                self._free[nbytes].append(ptr)
                return
        self._lib.epa_host_free(ptr)

    def close(self) -> None:
        with self._lock:
            self._closed = True
            ptrs = [p for v in self._free.values() for p in v]
            self._free.clear()
        for p in ptrs:
            self._lib.epa_host_free(p)


class DevicePool:
    """Low-level pool: numpy in, list-of-numpy out, in `_state_keys` order."""

    _SMALL_BATCH_BYTES = 256 * 1024
    key_players: list[int] | None = None

    def __init__(
        self,
        family: str,
        num_envs: int,
        batch_size: int = 0,
        seed: int = 42,
        env_seed: Sequence[int] | None = None,
        max_episode_steps: int = 0,
        device: int = 0,
        env_id_offset: int = 0,
        params: dict[str, float] | None = None,
    ) -> None:
        self._lib = native.lib()
        self.family = family
        self.num_envs = int(num_envs)
        self.batch_size = int(batch_size) if batch_size else int(num_envs)
        self.env_id_offset = int(env_id_offset)
        self.device = int(device)
        cfg, keep = native.make_config(
            num_envs, batch_size, seed, env_seed, max_episode_steps, device,
            env_id_offset, params,
        )
        h = self._create(family, cfg, params)
        del keep
        self._h = h
        # per state key: P if its rows carry the leading player dimension (multi-player families), else 1
        if self.key_players is None:
            self.key_players = [1] * len(self.state_keys)
        self.players = max(self.key_players)
        self._pending: collections.deque[int] = collections.deque()
        # per pending send / reset, the pinned block named at send time (None: recv takes one)
        self._posted: collections.deque[Any] = collections.deque()
        self._is_sync = self.batch_size == self.num_envs
        self._blocks = _PinnedBlocks(self._lib)
        self._step_ptrs = None  # step_device: reusable ctypes output array + cache of pointer lists
        self._layouts: dict[int, tuple[list[int], int]] = {}

    def _create(self, family: str, cfg: Any, params: dict[str, float] | None) -> ctypes.c_void_p:
        """epa_create + the key tables (overridden by families with their own constructor)."""
        self.state_keys = native.describe(family, params, "state")
        self.key_players = native.describe_state_players(family, params)
        self.action_keys = native.describe(family, params, "action")
        self.action_dtype = self.action_keys[-1][1]
        self.action_shape = self.action_keys[-1][2]
        h = ctypes.c_void_p()
        native.check(
            self._lib.epa_create(family.encode(), ctypes.byref(cfg), ctypes.byref(h))
        )
        return h

    # -- host path ---------------------------------------------------------
    def send(self, env_id: np.ndarray, action: np.ndarray, post_block: bool = True) -> None:
        env_id = np.ascontiguousarray(env_id, dtype=np.int32)
        action = np.ascontiguousarray(action, dtype=self.action_dtype)
        k = int(env_id.shape[0])
        want = (k, *self.action_shape)
        if action.size != int(np.prod(want)):
            raise RuntimeError(
                f"Expected action of shape {want}, got {action.shape}"
            )
        # A whole-pool step of a sync pool names the block its results shall land in NOW (epa_send_into): the step
        # kernel then writes them straight into it and recv only waits for the kernel.  Whether the engine takes the
        # offer (ids in order, pinned block, "direct_out") is its business: recv hands the same block to
        # epa_recv_block either way.
        block = None
        if post_block and k == (self.num_envs if self._is_sync else self.batch_size):
            _, total = self._layout(k)
            if total >= self._SMALL_BATCH_BYTES:
                block = self._blocks.take(total)
        if block is not None:
            native.check(self._lib.epa_send_into(self._h, env_id.ctypes.data, k, action.ctypes.data,
                                                 block.ctypes.data, block.nbytes))
        else:
            native.check(
                self._lib.epa_send(self._h, env_id.ctypes.data, k, action.ctypes.data)
            )
        if k > 0:  # an empty send enqueues nothing (Pool::Send returns early)
            self._pending.append(k)
            self._posted.append(block)

    def pop_pending(self) -> None:
        """A batch was received through another recv entry point (epa_recv_into of the sharded pool)."""
        self._pending.popleft()
        if self._posted:
            self._posted.popleft()

    def reset(self, env_ids: np.ndarray) -> None:
        env_ids = np.ascontiguousarray(env_ids, dtype=np.int32)
        k = int(env_ids.shape[0])
        native.check(self._lib.epa_reset(self._h, env_ids.ctypes.data, k))
        if k > 0:
            self._pending.append(k)
            self._posted.append(None)

    def _layout(self, rows: int) -> tuple[list[int], int]:
        lay = self._layouts.get(rows)
        if lay is None:
            n = len(self.state_keys)
            offs = (ctypes.c_size_t * n)()
            total = ctypes.c_size_t(0)
            native.check(self._lib.epa_recv_layout(self._h, rows, offs, n, ctypes.byref(total)))
            lay = ([int(o) for o in offs], int(total.value))
            self._layouts[rows] = lay
        return lay

    def recv(self) -> list[np.ndarray]:
        """One device->host copy into a pinned block; the returned arrays are
        views of that block (no host-side memcpy) and own it jointly."""
        if self._is_sync:
            cap = self._pending[0] if self._pending else self.num_envs
        else:
            cap = self.batch_size
        n = len(self.state_keys)
        _, total = self._layout(cap)
        small = total < self._SMALL_BATCH_BYTES
        k = ctypes.c_int32(0)
        if small:
            # tiny batches: fresh pageable arrays + epa_recv's memcpy out of its own
            # pinned landing buffer is cheaper than block bookkeeping
            outs = [np.empty((cap, *shape), dtype=dtype) for _, dtype, shape in self.state_keys]
            ptrs = (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs])
            native.check(self._lib.epa_recv(self._h, ptrs, n, cap, ctypes.byref(k)))
        else:
            # the block named at send time for exactly these rows (async: the oldest send is a whole, untouched batch)
            block = None
            if self._posted and (self._is_sync or (self._pending and self._pending[0] == cap)):
                block = self._posted[0]
            if block is None or block.nbytes < total:
                block = self._blocks.take(total)
            offs = (ctypes.c_size_t * n)()
            native.check(
                self._lib.epa_recv_block(self._h, block.ctypes.data, block.nbytes, offs, n,
                                         ctypes.byref(k))
            )
        if self._is_sync:
            if self._pending:
                self._pending.popleft()
            if self._posted:
                self._posted.popleft()
        else:
            # async: rows drain across submissions in order
            left = k.value
            while left > 0 and self._pending:
                if self._pending[0] <= left:
                    left -= self._pending.popleft()
                    if self._posted:
                        self._posted.popleft()
                else:
                    self._pending[0] -= left
                    left = 0
        rows = k.value
        if small:
            return self.player_rows(outs if rows == cap else [o[:rows] for o in outs])
        # one view per key straight onto the block (each holds the block as its base: the block goes back to the free
        # list when the last of them dies)
        return self.player_rows([np.ndarray((rows, *shape), dtype=dtype, buffer=block, offset=int(off))
                                 for (_, dtype, shape), off in zip(self.state_keys, offs)])

    def view_shape(self, i: int, rows: int) -> tuple[int, ...]:
        """Shape of state key i for a batch of `rows` env rows as recv hands it out: a per-player key's [rows, P, ...]
        block as the reference's [rows * P, ...] player rows (env-major: the P rows of an env are adjacent)."""
        shape, p = self.state_keys[i][2], self.key_players[i]
        return (rows * p, *shape[1:]) if p > 1 else (rows, *shape)

    def player_rows(self, outs: list[np.ndarray]) -> list[np.ndarray]:
        """[rows, ...] per-env arrays in state key order -> the arrays recv returns (views, no copy)."""
        if self.players == 1:
            return outs
        return [o.reshape(self.view_shape(i, o.shape[0])) for i, o in enumerate(outs)]

    def recv_dict(self) -> dict[str, np.ndarray]:
        return {k[0]: v for k, v in zip(self.state_keys, self.recv())}

    # -- device path ---------------------------------------------------------
    def send_device(self, d_action: int | None, k: int | None = None,
                    d_env_id: int | None = None, wait_event: int | None = None) -> None:
        """`d_action` / `d_env_id` are raw device addresses (ints); `wait_event` is a
        hipEvent_t (int) the producer of those buffers recorded on its stream."""
        k = self.num_envs if k is None else int(k)
        native.check(
            self._lib.epa_send_device(
                self._h, ctypes.c_void_p(d_env_id), k, ctypes.c_void_p(d_action),
                ctypes.c_void_p(wait_event),
            )
        )

    def wait_stream(self, producer_stream: int | None) -> None:
        """Order the pool's stream behind everything enqueued on `producer_stream`
        (raw hipStream_t, e.g. torch.cuda.current_stream().cuda_stream)."""
        native.check(self._lib.epa_wait_stream(self._h, ctypes.c_void_p(producer_stream)))

    def consumer_wait(self, consumer_stream: int | None) -> None:
        """`consumer_stream` waits for the batch the last recv_device handed out."""
        native.check(self._lib.epa_consumer_wait(self._h, ctypes.c_void_p(consumer_stream)))

    def recv_device(self) -> tuple[list[int], int]:
        """Device pointers of the next batch (one per state key) and its row count.  Does not wait for the batch's
        kernel, so a pool error word (see torch_interop) set by that kernel raises at a later recv or at
        `synchronize()`, not here."""
        n = len(self.state_keys)
        ptrs = (ctypes.c_void_p * n)()
        k = ctypes.c_int32(0)
        native.check(self._lib.epa_recv_device(self._h, ptrs, n, ctypes.byref(k)))
        return [int(p) if p else 0 for p in ptrs], k.value

    def step_device(self, d_action: int | None, k: int | None = None, d_env_id: int | None = None,
                    wait_event: int | None = None) -> tuple[tuple[int, ...], int]:
        """send_device + recv_device in one library call (the sync `step()` of the device path).  A pool hands out
        its result blocks in rotation, so the pointer tuples are cached per block (immutable: the same object is
        returned for every step on that block)."""
        k = self.num_envs if k is None else int(k)
        n = len(self.state_keys)
        if self._step_ptrs is None:
            self._step_ptrs, self._step_k, self._step_cache = (ctypes.c_void_p * n)(), ctypes.c_int32(0), {}
        ptrs = self._step_ptrs
        rc = self._lib.epa_step_device(self._h, d_env_id, k, d_action, wait_event, ptrs, n, ctypes.byref(self._step_k))
        if rc:
            native.check(rc)
        key = (ptrs[0], ptrs[n - 1])  # first and last section: the block and its layout
        out = self._step_cache.get(key)
        if out is None:
            out = self._step_cache[key] = tuple(int(p) if p else 0 for p in ptrs)
        return out, self._step_k.value

    @property
    def stream(self) -> int:
        return int(self._lib.epa_stream(self._h) or 0)

    def synchronize(self) -> None:
        native.check(self._lib.epa_synchronize(self._h))

    def set_timing(self, on: bool | int) -> None:
        """False / 0 off; True / 1 an event pair per launch; 2 one pair around the window
        (first launch .. kernel_time_ms()), nothing inserted between the launches."""
        native.check(self._lib.epa_set_timing(self._h, int(on)))

    def kernel_time_ms(self) -> tuple[float, int]:
        ms = ctypes.c_double(0)
        n = ctypes.c_int32(0)
        native.check(
            self._lib.epa_kernel_time_ms(self._h, ctypes.byref(ms), ctypes.byref(n))
        )
        return ms.value, n.value

    # -- test hooks ----------------------------------------------------------
    def state_dim(self) -> int:
        d = ctypes.c_int32(0)
        native.check(self._lib.epa_state_dim(self._h, ctypes.byref(d)))
        return d.value

    def get_state(self, env_ids: Any = None) -> np.ndarray:
        ids = self._ids(env_ids)
        out = np.empty((len(ids), self.state_dim()), dtype=np.float64)
        native.check(
            self._lib.epa_get_state(self._h, ids.ctypes.data, len(ids), out.ctypes.data)
        )
        return out

    def set_state(self, state: np.ndarray, env_ids: Any = None) -> None:
        ids = self._ids(env_ids)
        state = np.ascontiguousarray(state, dtype=np.float64)
        assert state.shape == (len(ids), self.state_dim()), state.shape
        native.check(
            self._lib.epa_set_state(self._h, ids.ctypes.data, len(ids), state.ctypes.data)
        )

    # -- render ----------------------------------------------------------------
    def render_size(self, width: int = 0, height: int = 0) -> tuple[int, int]:
        """(width, height) of the frames `render` returns: a width / height <= 0 is the env's default.  Raises
        RuntimeError("render not implemented for this environment") for a family that does not render."""
        w, h = ctypes.c_int32(0), ctypes.c_int32(0)
        native.check(self._lib.epa_render_size(self._h, int(width), int(height), ctypes.byref(w), ctypes.byref(h)))
        return w.value, h.value

    def render(self, env_ids: Any, width: int = 0, height: int = 0, camera_id: int = -1) -> np.ndarray:
        """uint8 [k, H, W, 3] RGB frames of the listed envs (global ids, duplicates allowed), painted on the device
        from the state every send so far has left them in; byte-identical with the reference's `render`."""
        ids = np.ascontiguousarray(env_ids, dtype=np.int32).reshape(-1)
        w, h = self.render_size(width, height)
        out = np.empty((len(ids), h, w, 3), dtype=np.uint8)
        native.check(self._lib.epa_render(self._h, ids.ctypes.data, len(ids), int(width), int(height),
                                          int(camera_id), out.ctypes.data))
        return out

    def render_device(self, d_out: int, env_ids: Any, width: int = 0, height: int = 0, camera_id: int = -1) -> None:
        """`render` into device memory at the raw address `d_out` (room for [k, H, W, 3] bytes, see `render_size`):
        enqueued on the pool's stream, nothing is copied to the host (torch_interop.render_device wraps it)."""
        ids = np.ascontiguousarray(env_ids, dtype=np.int32).reshape(-1)
        native.check(self._lib.epa_render_device(self._h, ids.ctypes.data, len(ids), int(width), int(height),
                                                 int(camera_id), ctypes.c_void_p(d_out)))

    # -- snapshot / restore / fork -----------------------------------------------
    def snapshot_bytes(self, k: int, rng: bool = True) -> int:
        """Bytes of a snapshot blob of `k` envs, with (`rng`) or without the generator section."""
        n = ctypes.c_size_t(0)
        native.check(self._lib.epa_snapshot_bytes(self._h, int(k), native.EPA_SNAP_RNG if rng else 0,
                                                  ctypes.byref(n)))
        return int(n.value)

    def snapshot(self, env_ids: Any = None, rng: bool = True) -> np.ndarray:
        """Everything that makes the listed envs (global ids; None: the whole pool) continue bit for bit, as an
        opaque uint8 blob: the flat state, with `rng` the generators, and the observation ring of frame_stack > 1.
        Shows each env after every send issued so far, received or not."""
        ids = self._ids(env_ids).reshape(-1)
        flags = native.EPA_SNAP_RNG if rng else 0
        n = ctypes.c_size_t(0)
        native.check(self._lib.epa_snapshot_bytes(self._h, len(ids), flags, ctypes.byref(n)))
        out = np.empty(int(n.value), dtype=np.uint8)
        native.check(self._lib.epa_snapshot(self._h, ids.ctypes.data, len(ids), flags, out.ctypes.data, out.nbytes))
        return out

    def _restore_ids(self, env_ids: Any, k: int) -> np.ndarray:
        if env_ids is None:  # ids 0 .. k-1 of this pool, k from the header
            return np.arange(self.env_id_offset, self.env_id_offset + k, dtype=np.int32)
        return np.ascontiguousarray(env_ids, dtype=np.int32).reshape(-1)

    def restore(self, blob: np.ndarray, env_ids: Any = None) -> None:
        """Put a snapshot's envs into the listed envs of this pool (None: envs 0 .. k-1, k from the blob).  The blob
        may come from any pool of the same family and frame_stack.  Takes effect before every later send."""
        blob = np.ascontiguousarray(blob)
        k, _ = native.snapshot_header(blob)
        ids = self._restore_ids(env_ids, k)
        native.check(self._lib.epa_restore(self._h, ids.ctypes.data, len(ids), blob.ctypes.data, blob.nbytes))

    def snapshot_device(self, d_blob: int, env_ids: Any = None, rng: bool = True) -> bytes:
        """`snapshot` into device memory at the raw address `d_blob` (16-byte aligned, `snapshot_bytes` long): only
        enqueued on the pool's stream.  Returns the blob's 64-byte header, which `restore_device` wants back."""
        ids = self._ids(env_ids).reshape(-1)
        header = ctypes.create_string_buffer(native.SNAP_HEADER_BYTES)
        native.check(self._lib.epa_snapshot_device(self._h, ids.ctypes.data, len(ids),
                                                   native.EPA_SNAP_RNG if rng else 0, ctypes.c_void_p(d_blob), header))
        return header.raw

    def restore_device(self, d_blob: int, header: bytes, env_ids: Any = None) -> None:
        """`restore` from device memory at the raw address `d_blob`; `header`: the blob's first 64 bytes on the host
        (the engine checks them without reading device memory)."""
        head = np.frombuffer(bytes(header), dtype=np.uint8)
        if head.nbytes < native.SNAP_HEADER_BYTES:
            raise ValueError(f"snapshot header of {head.nbytes} bytes is shorter than a header")
        ids = self._restore_ids(env_ids, int(head[20:24].view("<i4")[0]))
        native.check(self._lib.epa_restore_device(self._h, ids.ctypes.data, len(ids), ctypes.c_void_p(d_blob),
                                                  head.ctypes.data))

    def fork(self, src: Any, dst: Any, rng: bool = True) -> None:
        """Env dst[i] becomes env src[i], on the device (global ids): `src` may repeat and overlap `dst`, `dst` must
        not repeat.  With `rng` the copies draw the same numbers from then on."""
        src = np.ascontiguousarray(src, dtype=np.int32).reshape(-1)
        dst = np.ascontiguousarray(dst, dtype=np.int32).reshape(-1)
        if len(src) != len(dst):
            raise ValueError(f"fork: {len(src)} source ids for {len(dst)} targets")
        native.check(self._lib.epa_fork(self._h, src.ctypes.data, dst.ctypes.data, len(src),
                                        native.EPA_SNAP_RNG if rng else 0))

    # -- playouts ----------------------------------------------------------------
    def playout(self, env_ids: Any = None, repeats: int = 1, max_plies: int = 0, seed: int = 0,
                commit: bool = False) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """`repeats` uniform-random playouts of every listed env (global ids; None: the whole pool) from the state
        every send so far has left it in, in one kernel launch (the PGX board games; RuntimeError("playout not
        implemented for this environment") elsewhere).  Returns (returns float32 [k, R, 2], plies int32 [k, R],
        status uint8 [k, R]: 0 the game is over, 1 stopped at `max_plies`; 0 = 256).  The picks depend on (seed,
        env id, repeat, ply) and the position only.  Nothing of the pool changes unless `commit` (repeats = 1, ids
        that do not repeat) writes the final states back, as if the plies had been stepped without rows."""
        ids = native.check_playout(self._ids(env_ids), repeats, max_plies, commit)
        k, r = len(ids), int(repeats)
        returns = np.empty((k, r, 2), dtype=np.float32)
        plies = np.empty((k, r), dtype=np.int32)
        status = np.empty((k, r), dtype=np.uint8)
        native.check(self._lib.epa_playout(self._h, ids.ctypes.data, k, r, int(max_plies),
                                           int(seed) & (2**64 - 1), native.EPA_PLAYOUT_COMMIT if commit else 0,
                                           returns.ctypes.data, plies.ctypes.data, status.ctypes.data))
        return returns, plies, status

    def playout_device(self, d_returns: int, d_plies: int, d_status: int, env_ids: Any = None, repeats: int = 1,
                       max_plies: int = 0, seed: int = 0, commit: bool = False) -> None:
        """`playout` into device memory at the raw addresses `d_returns` (8 k R bytes, 8-byte aligned), `d_plies`
        (4 k R bytes, 4-byte aligned) and `d_status` (k R bytes): only enqueued on the pool's stream, nothing is
        copied to the host (torch_interop.playout_device wraps it)."""
        ids = native.check_playout(self._ids(env_ids), repeats, max_plies, commit)
        native.check(self._lib.epa_playout_device(self._h, ids.ctypes.data, len(ids), int(repeats), int(max_plies),
                                                  int(seed) & (2**64 - 1),
                                                  native.EPA_PLAYOUT_COMMIT if commit else 0,
                                                  ctypes.c_void_p(d_returns), ctypes.c_void_p(d_plies),
                                                  ctypes.c_void_p(d_status)))

    # -- tree search -------------------------------------------------------------
    def search_actions(self) -> int:
        """A, the width of a search's result rows, as the engine states it; a family without search raises."""
        n = ctypes.c_int32(0)
        native.check(self._lib.epa_search_actions(self._h, ctypes.byref(n)))
        if n.value <= 0:
            raise RuntimeError("search not implemented for this environment")
        return int(n.value)

    def search(self, env_ids: Any = None, simulations: int = 64, leaf_playouts: int = 8, c_puct: float = 1.25,
               max_plies: int = 0, seed: int = 0) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """A tree search from the current position of every listed env (global ids; None: the whole pool), in one
        kernel launch, one wave per root (the PGX board games; RuntimeError("search not implemented for this
        environment") elsewhere): `simulations` rounds of PUCT selection with uniform priors, every new leaf valued
        by the sum of `leaf_playouts` random playouts -- repeats t * leaf_playouts + r of `playout(seed)` for
        simulation t.  Returns (visits int32 [k, A], returns int32 [k, A]: the summed playout returns through each
        root action, seen from the root's mover, action int32 [k]: the most visited action, the lowest on ties; -1
        and zeros for an env that is over).  Nothing of the pool changes."""
        ids = native.check_search(self._ids(env_ids), simulations, leaf_playouts, c_puct, max_plies)
        k, a = len(ids), self.search_actions()
        visits = np.empty((k, a), dtype=np.int32)
        returns = np.empty((k, a), dtype=np.int32)
        action = np.empty(k, dtype=np.int32)
        native.check(self._lib.epa_search(self._h, ids.ctypes.data, k, int(simulations), int(leaf_playouts),
                                          float(c_puct), int(max_plies), int(seed) & (2**64 - 1),
                                          visits.ctypes.data, returns.ctypes.data, action.ctypes.data))
        return visits, returns, action

    def search_device(self, d_visits: int, d_returns: int, d_action: int, env_ids: Any = None, simulations: int = 64,
                      leaf_playouts: int = 8, c_puct: float = 1.25, max_plies: int = 0, seed: int = 0) -> None:
        """`search` into device memory at the raw addresses `d_visits`, `d_returns` (4 k A bytes each) and `d_action`
        (4 k bytes), all 4-byte aligned: only enqueued on the pool's stream, nothing is copied to the host
        (torch_interop.search_device wraps it)."""
        ids = native.check_search(self._ids(env_ids), simulations, leaf_playouts, c_puct, max_plies)
        native.check(self._lib.epa_search_device(self._h, ids.ctypes.data, len(ids), int(simulations),
                                                 int(leaf_playouts), float(c_puct), int(max_plies),
                                                 int(seed) & (2**64 - 1), ctypes.c_void_p(d_visits),
                                                 ctypes.c_void_p(d_returns), ctypes.c_void_p(d_action)))

    # -- exact solve -------------------------------------------------------------
    def solve_actions(self) -> int:
        """A, the width of a solve's q rows (a family with solve has search: the engine states A once); a family
        without raises."""
        n = ctypes.c_int32(0)
        native.check(self._lib.epa_search_actions(self._h, ctypes.byref(n)))
        if n.value <= 0:
            raise RuntimeError("solve not implemented for this environment")
        return int(n.value)

    def solve(self, env_ids: Any = None, depth: int = 0, max_nodes: int = 1 << 20,
              table_bits: int = 0) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """The exact minimax value of the current position of every listed env (global ids; None: the whole pool),
        by alpha-beta in one kernel launch, one wave per root (the PGX board games; RuntimeError("solve not
        implemented for this environment") elsewhere).  `depth` D: the horizon in plies (a position the horizon cuts
        counts 0); 0: to the end of the game.  Returns (value int8 [k]: the maximum of q, q int8 [k, A]: the value
        through each legal root action, seen from the root's mover, -128 for an illegal one, action int32 [k]: the
        lowest action of that value, status uint8 [k]: 0 solved, 1 given up after more than `max_nodes` positions, 2
        the env is over -- then value 0, action -1, q -128 --, nodes int64 [k]: the positions visited).  Nothing of the
        pool changes.  `table_bits` = b, 1 .. 16 (epa_solve_table): every lane of a root's wave keeps a private
        transposition table of 2^b entries for the call, so a position it meets again is not searched again; the same
        values wherever both solve the row, other `nodes`; 0: no tables, today's call."""
        ids = native.check_solve(self._ids(env_ids), depth, max_nodes, table_bits)
        k, a = len(ids), self.solve_actions()
        value = np.empty(k, dtype=np.int8)
        q = np.empty((k, a), dtype=np.int8)
        action = np.empty(k, dtype=np.int32)
        status = np.empty(k, dtype=np.uint8)
        nodes = np.empty(k, dtype=np.int64)
        native.check(self._lib.epa_solve_table(self._h, ids.ctypes.data, k, int(depth), int(max_nodes),
                                               int(table_bits), value.ctypes.data, q.ctypes.data, action.ctypes.data,
                                               status.ctypes.data, nodes.ctypes.data))
        return value, q, action, status, nodes

    def solve_device(self, d_value: int, d_q: int, d_action: int, d_status: int, d_nodes: int, env_ids: Any = None,
                     depth: int = 0, max_nodes: int = 1 << 20, table_bits: int = 0) -> None:
        """`solve` into device memory at the raw addresses `d_value` (k bytes), `d_q` (k A bytes), `d_action` (4 k
        bytes, 4-byte aligned), `d_status` (k bytes) and `d_nodes` (8 k bytes, 8-byte aligned): only enqueued on the
        pool's stream, nothing is copied to the host (torch_interop.solve_device wraps it)."""
        ids = native.check_solve(self._ids(env_ids), depth, max_nodes, table_bits)
        native.check(self._lib.epa_solve_table_device(self._h, ids.ctypes.data, len(ids), int(depth), int(max_nodes),
                                                      int(table_bits), ctypes.c_void_p(d_value), ctypes.c_void_p(d_q),
                                                      ctypes.c_void_p(d_action), ctypes.c_void_p(d_status),
                                                      ctypes.c_void_p(d_nodes)))

    # -- guided tree search --------------------------------------------------------
    def guided_shape(self) -> tuple[int, int, int, int]:
        """(H, W, C, A) of a guided search's leaf arrays, as the engine states them; a family without raises."""
        out = (ctypes.c_int32 * 4)()
        native.check(self._lib.epa_guided_shape(self._h, out))
        if out[3] <= 0:
            raise RuntimeError("guided search not implemented for this environment")
        return int(out[0]), int(out[1]), int(out[2]), int(out[3])

    def _guided_leaves(self, k: int, width: int = 0) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        h, w, c, a = self.guided_shape()
        lead = (k, width) if width else (k,)  # (a wide session's leaves carry the slot axis)
        return (np.empty(lead + (h, w, c), dtype=np.bool_), np.empty(lead + (a,), dtype=np.bool_),
                np.empty(lead, dtype=np.uint8))

    def guided_begin(self, env_ids: Any = None, simulations: int = 64, c_puct: float = 1.25,
                     nodes: int = 0, width: Any = None, tactics: int = 0,
                     tactics_nodes: int = native.GUIDED_TACTICS_NODES,
                     prove: bool = False) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Opens the pool's guided-search session (the PGX board games; RuntimeError("guided search not implemented
        for this environment") elsewhere) on the current positions of the listed envs (global ids; None: the whole
        pool), replacing any earlier one: a PUCT search whose tree stays on the device and that stops at every new
        leaf for the caller's priors and value (include/envpool_amd.h: epa_guided_begin has the contract).  Returns
        the first leaves (obs bool [k, H, W, C] of the seat to move, mask bool [k, A], status uint8 [k]: 0 evaluate,
        1 a finished game, 2 nothing pending).  Nothing of the pool changes, and later steps of the pool change
        nothing in the session.  `nodes`: the node capacity per root, simulations + 1 .. 8192 (0: simulations + 1),
        the room `guided_reroot` needs to keep a subtree and grow it.  `width` = W, 1 .. 32, opens a WIDE session
        (epa_guided_begin_wide): W slots per root, up to W leaves per root and advance, steered apart by virtual
        losses; every leaf array and the rows of `guided_advance` then carry a slot axis ([k, W, ...]), a slot of
        status 2 has nothing pending, and the round is complete when all statuses are 2.  None: a plain session.
        `tactics` = D, 1 .. 16, turns on the exact leaf status (epa_guided_begin_tactics): every new leaf other than
        the root is solved D plies deep with at most `tactics_nodes` positions, and a leaf that is a forced win or loss
        comes back with status 1 and backs up +-1 for good; 0: off, today's calls.
        `prove` = True turns on proven values (epa_guided_begin_prove): exact values of finished games and decided
        leaves climb the tree, proven subtrees are closed, a proven root ends its round early, and the result's action
        is never a move proven to lose while another is not; `guided_proof` reads the proofs.  False: today's calls."""
        ids = native.check_guided(self._ids(env_ids), simulations, c_puct)
        cap = native.check_guided_nodes(simulations, nodes)
        width = native.check_guided_width(width)
        tactics, tactics_nodes = native.check_guided_tactics(tactics, tactics_nodes)
        prove = native.check_guided_prove(prove)
        self.guided_shape()
        obs, mask, status = self._guided_leaves(len(ids), width)
        native.check(self._lib.epa_guided_begin_prove(
            self._h, ids.ctypes.data, len(ids), int(simulations), int(nodes or 0), width, float(c_puct), tactics,
            tactics_nodes, native.GUIDED_PROVE if prove else 0, obs.ctypes.data, mask.ctypes.data, status.ctypes.data))
        self._guided_k, self._guided_policy, self._guided_nodes = len(ids), "puct", cap
        self._guided_width = width
        return obs, mask, status

    def guided_reroot(self, actions: Any, simulations: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Tree reuse, after the round's last advance: root i's tree becomes the subtree under `actions[i]` (int32
        [k], the move played), compacted in place on the device; a move the search never tried gives a fresh tree on
        the position behind it, and a root whose game that move ends is over from then on.  The next round has
        `simulations` simulations (simulations + 1 <= the session's nodes) and starts with the new roots as its
        leaves, which are returned as `guided_begin` returns its own; the kept visits count in `guided_result`.
        ValueError before any launch: no session, a Gumbel session, a round that is not complete (a wide session: a
        slot that is still pending), another number of rows, an action outside 0 .. A-1.  A wide session takes one
        action per root, too; afterwards slot 0 holds the new root and the other slots are idle."""
        k = self._guided_open("guided_reroot", "puct")
        actions = native.check_guided_reroot(actions, k, self.guided_shape()[3], simulations,
                                             getattr(self, "_guided_nodes", native.GUIDED_MAX_NODES))
        obs, mask, status = self._guided_leaves(k, getattr(self, "_guided_width", 0))
        native.check(self._lib.epa_guided_reroot(self._h, actions.ctypes.data, k, int(simulations), obs.ctypes.data,
                                                 mask.ctypes.data, status.ctypes.data))
        return obs, mask, status

    def _guided_open(self, what: str, policy: str) -> int:
        """The open session's k; ValueError without a session, or with one of the other policy (before any native
        call)."""
        k = getattr(self, "_guided_k", None)
        if k is None:
            raise ValueError(f"{what}: the pool has no guided-search session")
        if getattr(self, "_guided_policy", "puct") != policy:
            other = "guided" if policy == "gumbel" else "gumbel"
            raise ValueError(f"{what}: the pool's session is a {'PUCT guided' if other == 'guided' else 'Gumbel'} "
                             f"search: use {other}_{what.split('_', 1)[1]}")
        return k

    def guided_advance(self, priors: Any, values: Any) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """One simulation of every root of the session, one launch: `priors` float32 [k, A] and `values` float32 [k]
        (for the seat that moves at the leaf) answer the leaves handed out last; returns the next leaves.  Call it
        simulations + 1 times.  Rows that are not finite, negative priors and values outside -1 .. 1 raise ValueError
        before any launch."""
        k = self._guided_open("guided_advance", "puct")
        width = getattr(self, "_guided_width", 0)
        if width:  # a wide session: rows [k, W, ..] or flattened, the leaves with the slot axis
            priors, values = native.check_guided_wide_rows(priors, values, k, width, self.guided_shape()[3])
        else:
            priors, values = native.check_guided_rows(priors, values, k, self.guided_shape()[3])
        obs, mask, status = self._guided_leaves(k, width)
        native.check(self._lib.epa_guided_advance(self._h, priors.ctypes.data, values.ctypes.data, len(values),
                                                  obs.ctypes.data, mask.ctypes.data, status.ctypes.data))
        return obs, mask, status

    def guided_result(self) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(visits int32 [k, A], values float32 [k, A]: the summed values through each root action, seen from the
        root's mover, action int32 [k]: the most visited legal action, the lowest on ties; -1 and zeros for an env
        that was over).  Valid any time after guided_begin, complete after simulations + 1 advances."""
        k = self._guided_open("guided_result", "puct")
        a = self.guided_shape()[3]
        visits = np.empty((k, a), dtype=np.int32)
        values = np.empty((k, a), dtype=np.float32)
        action = np.empty(k, dtype=np.int32)
        native.check(self._lib.epa_guided_result(self._h, visits.ctypes.data, values.ctypes.data, action.ctypes.data))
        return visits, values, action

    def guided_decided(self, with_nodes: bool = False) -> Any:
        """int32 [k]: the leaves the exact leaf status decided per root since guided_begin (zeros without `tactics`); a
        reroot does not reduce it.  with_nodes: (decided, int64 [k] positions the solver visited per root)."""
        k = self._guided_open("guided_decided", "puct")
        decided, nodes = np.empty(k, dtype=np.int32), np.empty(k, dtype=np.int64)
        native.check(self._lib.epa_guided_decided(self._h, decided.ctypes.data, nodes.ctypes.data))
        return (decided, nodes) if with_nodes else decided

    def guided_proof(self) -> tuple[np.ndarray, np.ndarray]:
        """Proven values (`prove=True`), at any time: (value int8 [k], the root's proven value for its mover; q int8
        [k, A], per legal root action the proven value of its child for the root's mover).  -128: unproven, no child,
        an illegal action, a root that is over -- and everywhere for a session without `prove`."""
        k = self._guided_open("guided_proof", "puct")
        value, q = np.empty(k, dtype=np.int8), np.empty((k, self.guided_shape()[3]), dtype=np.int8)
        native.check(self._lib.epa_guided_proof(self._h, value.ctypes.data, q.ctypes.data))
        return value, q

    def guided_proof_device(self, d_value: int, d_q: int) -> None:
        """`guided_proof` into device memory (int8 [k] and int8 [k, A]): only enqueued."""
        self._guided_open("guided_proof", "puct")
        native.check(self._lib.epa_guided_proof_device(self._h, ctypes.c_void_p(d_value), ctypes.c_void_p(d_q)))

    def guided_decided_device(self, d_decided: int, d_nodes: int = 0) -> None:
        """`guided_decided` into device memory (int32 [k]; `d_nodes`: int64 [k] or 0): only enqueued."""
        self._guided_open("guided_decided", "puct")
        native.check(self._lib.epa_guided_decided_device(self._h, ctypes.c_void_p(d_decided),
                                                         ctypes.c_void_p(d_nodes or None)))

    def guided_end(self) -> None:
        """Closes the session (of either policy) and releases its device memory; ValueError without one."""
        native.check(self._lib.epa_guided_end(self._h))
        self._guided_k = None

    def guided_begin_device(self, d_obs: int, d_mask: int, d_status: int, env_ids: Any = None, simulations: int = 64,
                            c_puct: float = 1.25, nodes: int = 0, width: Any = None, tactics: int = 0,
                            tactics_nodes: int = native.GUIDED_TACTICS_NODES, prove: bool = False) -> int:
        """`guided_begin` with the leaves written to device memory at the raw addresses `d_obs` (k H W C bytes),
        `d_mask` (k A bytes) and `d_status` (k bytes): only enqueued on the pool's stream.  Returns k.  With `width`
        = W the arrays have k W rows, and so have those of `guided_advance_device` (its `k` is k W) and of
        `guided_reroot_device` (whose `k` stays the number of roots)."""
        ids = native.check_guided(self._ids(env_ids), simulations, c_puct)
        cap = native.check_guided_nodes(simulations, nodes)
        width = native.check_guided_width(width)
        tactics, tactics_nodes = native.check_guided_tactics(tactics, tactics_nodes)
        prove = native.check_guided_prove(prove)
        native.check(self._lib.epa_guided_begin_prove_device(
            self._h, ids.ctypes.data, len(ids), int(simulations), int(nodes or 0), width, float(c_puct), tactics,
            tactics_nodes, native.GUIDED_PROVE if prove else 0, ctypes.c_void_p(d_obs), ctypes.c_void_p(d_mask),
            ctypes.c_void_p(d_status)))
        self._guided_k, self._guided_policy, self._guided_nodes = len(ids), "puct", cap
        self._guided_width = width
        return len(ids)

    def guided_reroot_device(self, d_actions: int, k: int, simulations: int, d_obs: int, d_mask: int,
                             d_status: int) -> None:
        """`guided_reroot` on device memory: `d_actions` (int32 [k], 4-byte aligned) is read by the kernel, which
        ends a root whose action is outside 0 .. A-1; the leaves are written at `d_obs`, `d_mask`, `d_status`; only
        enqueued."""
        self._guided_open("guided_reroot", "puct")
        native.check_guided_reroot(None, k, 0, simulations, getattr(self, "_guided_nodes", native.GUIDED_MAX_NODES),
                                   device=True)
        native.check(self._lib.epa_guided_reroot_device(self._h, ctypes.c_void_p(d_actions), int(k), int(simulations),
                                                        ctypes.c_void_p(d_obs), ctypes.c_void_p(d_mask),
                                                        ctypes.c_void_p(d_status)))

    def guided_advance_device(self, d_priors: int, d_values: int, k: int, d_obs: int, d_mask: int,
                              d_status: int) -> None:
        """`guided_advance` on device memory: `d_priors` (float32 [k, A]) and `d_values` (float32 [k]), 4-byte
        aligned, are read by the kernel, which treats entries outside their range as 0; only enqueued."""
        native.check(self._lib.epa_guided_advance_device(self._h, ctypes.c_void_p(d_priors), ctypes.c_void_p(d_values),
                                                         int(k), ctypes.c_void_p(d_obs), ctypes.c_void_p(d_mask),
                                                         ctypes.c_void_p(d_status)))

    def guided_result_device(self, d_visits: int, d_values: int, d_action: int) -> None:
        """`guided_result` into device memory (4 k A, 4 k A and 4 k bytes, 4-byte aligned); only enqueued."""
        native.check(self._lib.epa_guided_result_device(self._h, ctypes.c_void_p(d_visits), ctypes.c_void_p(d_values),
                                                        ctypes.c_void_p(d_action)))

    # -- Gumbel search: the guided-search session's second policy ------------------
    def gumbel_actions(self) -> int:
        """A of a Gumbel search's rows; a family without raises."""
        out = (ctypes.c_int32 * 4)()
        native.check(self._lib.epa_guided_shape(self._h, out))
        if out[3] <= 0:
            raise RuntimeError("gumbel search not implemented for this environment")
        return int(out[3])

    def _gumbel_begin(self, form: str, ids: np.ndarray, simulations: int, considered: int, batch: int,
                      c_visit: float, c_scale: float, *arrays: Any) -> None:
        """The native begin of a Gumbel session, host ("") or "_device" form, `arrays` being its noise, obs, mask and
        status.  A plain session keeps an entry point of its own: epa_gumbel_begin_batch takes a batch of 1 .. 32 and
        refuses 0."""
        head = (self._h, ids.ctypes.data, len(ids), int(simulations), considered)
        tail = (float(c_visit), float(c_scale)) + arrays
        if batch:
            native.check(getattr(self._lib, "epa_gumbel_begin_batch" + form)(*head, batch, *tail))
        else:
            native.check(getattr(self._lib, "epa_gumbel_begin" + form)(*head, *tail))

    def gumbel_begin(self, gumbel: Any, env_ids: Any = None, simulations: int = 32, max_considered: int = 16,
                     c_visit: float = 50.0, c_scale: float = 0.1,
                     batch: Any = None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Opens the pool's guided-search session with the Gumbel policy (include/envpool_amd.h: epa_gumbel_begin has
        the contract), replacing any earlier session of either policy: Gumbel top-`max_considered` sampling with
        sequential halving at the root, the caller's logits and values at every new leaf.  `gumbel` float32 [k, A] is
        the caller's Gumbel(0, 1) noise per root action (zeros: the noise-free evaluation mode); the library draws no
        random numbers.  Returns the first leaves as `guided_begin` does.  Nothing of the pool changes.  `batch` = B,
        1 .. 32, opens a BATCH session (epa_gumbel_begin_batch): B slots per root, and every advance makes up to B
        simulations of the root's current level of sequential halving, chosen together from one scoring of the root;
        every leaf array and the rows of `gumbel_advance` then carry a slot axis ([k, B, ...]), a slot of status 2
        has nothing pending, and the round is complete when all statuses are 2.  None: a plain session."""
        ids = native.check_gumbel(self._ids(env_ids), simulations, max_considered, c_visit, c_scale)
        batch = native.check_gumbel_batch(batch)
        a = self.gumbel_actions()
        gumbel = native.check_gumbel_noise(gumbel, len(ids), a)
        obs, mask, status = self._guided_leaves(len(ids), batch)
        self._gumbel_begin("", ids, simulations, min(int(max_considered), a), batch, c_visit, c_scale,
                           gumbel.ctypes.data, obs.ctypes.data, mask.ctypes.data, status.ctypes.data)
        self._guided_k, self._guided_policy, self._gumbel_batch = len(ids), "gumbel", batch
        return obs, mask, status

    def gumbel_advance(self, logits: Any, values: Any) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """One simulation of every root of the Gumbel session, one launch: `logits` float32 [k, A] (any sign) and
        `values` float32 [k] (for the seat that moves at the leaf) answer the leaves handed out last; returns the next
        leaves.  Call it simulations + 1 times.  Rows that are not finite, logits above 1e30 in magnitude and values
        outside -1 .. 1 raise ValueError before any launch.  A batch session takes [k, B, A] and [k, B] (or the
        flattened rows), answers every pending slot and returns leaves with the slot axis; call it until every
        status is 2."""
        k = self._guided_open("gumbel_advance", "gumbel")
        batch = getattr(self, "_gumbel_batch", 0)
        if batch:  # a batch session: rows [k, B, ..] or flattened, the leaves with the slot axis
            logits, values = native.check_gumbel_batch_rows(logits, values, k, batch, self.guided_shape()[3])
        else:
            logits, values = native.check_gumbel_rows(logits, values, k, self.guided_shape()[3])
        obs, mask, status = self._guided_leaves(k, batch)
        native.check(self._lib.epa_gumbel_advance(self._h, logits.ctypes.data, values.ctypes.data, len(values),
                                                  obs.ctypes.data, mask.ctypes.data, status.ctypes.data))
        return obs, mask, status

    def gumbel_result(self) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """(visits int32 [k, A], values float32 [k, A], action int32 [k]: the recommended move -- the best of the most
        visited root actions by gumbel + logit + sigma(q); -1 for an env that was over --, weights float32 [k, A]: the
        improved policy softmax(logits + sigma(completed q)) of the root, the training target).  Valid any time after
        gumbel_begin, complete after simulations + 1 advances (a batch session: when every status is 2).  One row per
        root, whatever the batch."""
        k = self._guided_open("gumbel_result", "gumbel")
        a = self.guided_shape()[3]
        visits = np.empty((k, a), dtype=np.int32)
        values = np.empty((k, a), dtype=np.float32)
        action = np.empty(k, dtype=np.int32)
        weights = np.empty((k, a), dtype=np.float32)
        native.check(self._lib.epa_gumbel_result(self._h, visits.ctypes.data, values.ctypes.data, action.ctypes.data,
                                                 weights.ctypes.data))
        return visits, values, action, weights

    def gumbel_begin_device(self, d_gumbel: int, d_obs: int, d_mask: int, d_status: int, env_ids: Any = None,
                            simulations: int = 32, max_considered: int = 16, c_visit: float = 50.0,
                            c_scale: float = 0.1, batch: Any = None) -> int:
        """`gumbel_begin` on device memory: the noise is read at the raw address `d_gumbel` (float32 [k, A], 4-byte
        aligned; the kernel takes entries that are not finite as 0) and the leaves are written at `d_obs`, `d_mask`
        and `d_status`: only enqueued on the pool's stream.  Returns k.  With `batch` = B the leaf arrays have k B
        rows, and so have those of `gumbel_advance_device` (its `k` is k B); the noise keeps k rows."""
        ids = native.check_gumbel(self._ids(env_ids), simulations, max_considered, c_visit, c_scale)
        batch = native.check_gumbel_batch(batch)
        a = self.gumbel_actions()
        self._gumbel_begin("_device", ids, simulations, min(int(max_considered), a), batch, c_visit, c_scale,
                           ctypes.c_void_p(d_gumbel), ctypes.c_void_p(d_obs), ctypes.c_void_p(d_mask),
                           ctypes.c_void_p(d_status))
        self._guided_k, self._guided_policy, self._gumbel_batch = len(ids), "gumbel", batch
        return len(ids)

    def gumbel_advance_device(self, d_logits: int, d_values: int, k: int, d_obs: int, d_mask: int,
                              d_status: int) -> None:
        """`gumbel_advance` on device memory: `d_logits` (float32 [k, A]) and `d_values` (float32 [k]), 4-byte
        aligned, are read by the kernel, which treats entries outside their range as 0; only enqueued."""
        self._guided_open("gumbel_advance", "gumbel")
        native.check(self._lib.epa_gumbel_advance_device(self._h, ctypes.c_void_p(d_logits), ctypes.c_void_p(d_values),
                                                         int(k), ctypes.c_void_p(d_obs), ctypes.c_void_p(d_mask),
                                                         ctypes.c_void_p(d_status)))

    def gumbel_result_device(self, d_visits: int, d_values: int, d_action: int, d_weights: int) -> None:
        """`gumbel_result` into device memory (4 k A, 4 k A, 4 k and 4 k A bytes, 4-byte aligned); only enqueued."""
        self._guided_open("gumbel_result", "gumbel")
        native.check(self._lib.epa_gumbel_result_device(self._h, ctypes.c_void_p(d_visits), ctypes.c_void_p(d_values),
                                                        ctypes.c_void_p(d_action), ctypes.c_void_p(d_weights)))

    # -- the built-in network (envpool_amd/pgx/net.py; csrc/pgx_net.hip.h) -------------
    def _net_rows(self, what: str, obs: Any, mask: Any, status: Any) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Leaf arrays as contiguous bytes [rows, F], [rows, A], [rows]; ValueError for shapes that are no rows of
        this pool's game."""
        h, w, c, a = self.guided_shape()
        status = np.ascontiguousarray(status).reshape(-1)
        rows = len(status)
        obs, mask = np.ascontiguousarray(obs), np.ascontiguousarray(mask)
        if obs.itemsize != 1 or mask.itemsize != 1 or status.itemsize != 1:
            raise ValueError(f"{what}: obs, mask and status must be bool or uint8 arrays")
        if rows < 1 or obs.size != rows * h * w * c or mask.size != rows * a:
            raise ValueError(f"{what}: obs {obs.shape} and mask {mask.shape} for {rows} rows of [{h}, {w}, {c}] "
                             f"and [{a}]")
        return obs, mask, status

    def net_eval(self, net: Any, obs: Any, mask: Any, status: Any,
                 priors: bool = False) -> tuple[np.ndarray, np.ndarray]:
        """One evaluation of the built-in network `net` (envpool_amd.pgx.net.Net) on leaf rows of this pool's game
        (epa_net_eval): (policy float32 [rows, A] -- logits, or with `priors` the softmax over the legal actions --,
        value float32 [rows]).  A row whose status is not 0 gets zeros."""
        obs, mask, status = self._net_rows("net_eval", obs, mask, status)
        a = self.guided_shape()[3]
        policy, value = np.empty((len(status), a), dtype=np.float32), np.empty(len(status), dtype=np.float32)
        native.check(self._lib.epa_net_eval(self._h, net._handle(self.device), len(status), 1 if priors else 0,
                                            obs.ctypes.data, mask.ctypes.data, status.ctypes.data,
                                            policy.ctypes.data, value.ctypes.data))
        return policy, value

    def net_eval_device(self, net: Any, rows: int, priors: bool, d_obs: int, d_mask: int, d_status: int,
                        d_policy: int, d_value: int) -> None:
        """`net_eval` on device memory at raw addresses (policy and value 4-byte aligned): only enqueued on the
        pool's stream."""
        self.guided_shape()
        native.check(self._lib.epa_net_eval_device(
            self._h, net._handle(self.device), int(rows), 1 if priors else 0, ctypes.c_void_p(d_obs),
            ctypes.c_void_p(d_mask), ctypes.c_void_p(d_status), ctypes.c_void_p(d_policy), ctypes.c_void_p(d_value)))

    def net_run(self, net: Any, leaves: tuple, advances: Any = None) -> tuple[tuple, int]:
        """The open session's round with `net` as its evaluator, enqueued from C++ (epa_net_run): `leaves` are the
        session's last (obs, mask, status); `advances`: that many pairs of evaluation and advance, None: until the
        round is complete.  A PUCT session is fed priors, a Gumbel session logits.  Returns (the new leaves, in the
        shapes of the old, the advances made)."""
        self.guided_shape()
        if getattr(self, "_guided_k", None) is None:
            raise ValueError("net_run: the pool has no guided-search session")
        advances = native.check_net_advances(advances)
        shapes = [np.asarray(x).shape for x in leaves]
        obs, mask, status = (x.copy() for x in self._net_rows("net_run", *leaves))
        made = ctypes.c_int32(0)
        native.check(self._lib.epa_net_run(self._h, net._handle(self.device), advances, obs.ctypes.data,
                                           mask.ctypes.data, status.ctypes.data, ctypes.byref(made)))
        return (obs.reshape(shapes[0]), mask.reshape(shapes[1]), status.reshape(shapes[2])), int(made.value)

    def net_run_device(self, net: Any, d_obs: int, d_mask: int, d_status: int, advances: Any = None) -> int:
        """`net_run` on the device arrays of the `_device` begin or reroot, in place: only enqueued, except that a
        wide or batch session with `advances=None` reads one device word per advance.  Returns the advances made."""
        self.guided_shape()
        if getattr(self, "_guided_k", None) is None:
            raise ValueError("net_run: the pool has no guided-search session")
        made = ctypes.c_int32(0)
        native.check(self._lib.epa_net_run_device(self._h, net._handle(self.device), native.check_net_advances(advances),
                                                  ctypes.c_void_p(d_obs), ctypes.c_void_p(d_mask),
                                                  ctypes.c_void_p(d_status), ctypes.byref(made)))
        return int(made.value)

    # -- self-play recorder -------------------------------------------------------
    def record_begin(self, capacity: int, max_plies: int = 0, symmetries: bool = False) -> tuple[int, int, int, int, int]:
        """Opens the pool's recorder (the PGX board games; RuntimeError("recorder not implemented for this
        environment") elsewhere): finished games become training samples in `capacity` rows of device memory
        (csrc/pgx_record.hip.h).  `max_plies`: staged plies per env, 0: 128.  `symmetries`: every board symmetry of
        each sample.  A pool has one recorder; a new one replaces it.  Returns (H, W, C, A, nsym)."""
        capacity, max_plies, symmetries = native.check_record(capacity, max_plies, symmetries)
        native.check(self._lib.epa_record_begin(self._h, capacity, max_plies,
                                                native.RECORD_SYMMETRIES if symmetries else 0))
        self.record_capacity = capacity  # (the rows of `record_view_device`'s arrays)
        return self.record_shape()

    def record_shape(self) -> tuple[int, int, int, int, int]:
        """(H, W, C, A, nsym) of the open recorder."""
        out = (ctypes.c_int32 * 5)()
        native.check(self._lib.epa_record_shape(self._h, out))
        return int(out[0]), int(out[1]), int(out[2]), int(out[3]), int(out[4])

    def record_add(self, policy: Any, env_ids: Any = None) -> None:
        """Stages the current position of every listed env (global ids that do not repeat; None: the whole pool) with
        row i of `policy` float32 [k, A] as its policy target -- before the step.  Envs that are over are skipped."""
        ids = native.check_record_ids("recorder add", self._ids(env_ids))
        policy = native.check_record_add(policy, len(ids), self.record_shape()[3])
        native.check(self._lib.epa_record_add(self._h, ids.ctypes.data, len(ids), policy.ctypes.data))

    def record_finish(self, reward: Any, done: Any, env_ids: Any = None) -> None:
        """After the step, with what it returned: reward float32 [k, 2] (or [2 k]) and done [k] of the listed envs.
        Every env whose game ended turns its staged plies into samples, in the call's row order."""
        ids = native.check_record_ids("recorder finish", self._ids(env_ids))
        reward, done = native.check_record_finish(reward, done, len(ids))
        native.check(self._lib.epa_record_finish(self._h, ids.ctypes.data, len(ids), reward.ctypes.data,
                                                 done.ctypes.data))

    def record_counters(self) -> np.ndarray:
        """int64 [5]: the sample count, then samples and games written, dropped_games and dropped_plies since begin."""
        out = np.zeros(5, dtype=np.int64)
        native.check(self._lib.epa_record_counters(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return out

    def record_drain(self) -> tuple[np.ndarray, ...]:
        """The samples so far -- (obs bool [n, H, W, C], mask bool [n, A], policy float32 [n, A], value float32 [n],
        ply int32 [n], env_id int32 [n], sym uint8 [n]) -- and the count back to 0."""
        h, w, c, a, _ = self.record_shape()
        n = int(self.record_counters()[0])
        out = (np.empty((n, h, w, c), dtype=np.bool_), np.empty((n, a), dtype=np.bool_),
               np.empty((n, a), dtype=np.float32), np.empty(n, dtype=np.float32), np.empty(n, dtype=np.int32),
               np.empty(n, dtype=np.int32), np.empty(n, dtype=np.uint8))
        got = ctypes.c_int32(0)
        native.check(self._lib.epa_record_drain(self._h, n, *[o.ctypes.data for o in out], ctypes.byref(got)))
        return out

    def record_discard(self, env_ids: Any = None) -> None:
        """Forgets the staged plies of the listed envs (None: of every env); only enqueued."""
        if env_ids is None:
            native.check(self._lib.epa_record_discard(self._h, None, 0))
            return
        ids = native.check_record_ids("recorder discard", self._ids(env_ids))
        native.check(self._lib.epa_record_discard(self._h, ids.ctypes.data, len(ids)))

    def record_add_device(self, d_policy: int, env_ids: Any = None) -> None:
        """`record_add` with the policy rows in device memory at the raw address `d_policy` (4 k A bytes, 4-byte
        aligned): only enqueued on the pool's stream.  The ids must not repeat."""
        ids = native.check_record_ids("recorder add", self._ids(env_ids))
        native.check(self._lib.epa_record_add_device(self._h, ids.ctypes.data, len(ids), ctypes.c_void_p(d_policy)))

    def record_finish_device(self, d_reward: int, d_done: int, env_ids: Any = None) -> None:
        """`record_finish` with reward (8 k bytes, 4-byte aligned) and done (k bytes) in device memory: only enqueued.
        The ids must not repeat."""
        ids = native.check_record_ids("recorder finish", self._ids(env_ids))
        native.check(self._lib.epa_record_finish_device(self._h, ids.ctypes.data, len(ids),
                                                        ctypes.c_void_p(d_reward), ctypes.c_void_p(d_done)))

    def record_view_device(self) -> tuple[list[int], int]:
        """The raw addresses of the seven sample arrays (over the full capacity) and of the device int32 count."""
        arrays = (ctypes.c_void_p * 7)()
        count = ctypes.c_void_p()
        native.check(self._lib.epa_record_view_device(self._h, arrays, ctypes.byref(count)))
        return [int(p) for p in arrays], int(count.value)

    def record_clear(self) -> None:
        """Sets the sample count to 0 (what `record_drain` does after its copy); only enqueued."""
        native.check(self._lib.epa_record_clear(self._h))

    def record_end(self) -> None:
        """Closes the recorder and releases its device memory; ValueError without one."""
        native.check(self._lib.epa_record_end(self._h))

    # -- rollout collector (csrc/rollout.hip.h) ----------------------------------------
    def rollout_obs_keys(self) -> list[int]:
        """Indices of the state keys a collector stores: the family's keys whose name starts with "obs"."""
        return [i for i, (name, _, _) in enumerate(self.state_keys) if i >= 8 and name.startswith("obs")]

    def rollout_row_bytes(self) -> tuple[int, int]:
        """(observation bytes, action bytes) per env and slot: what `native.check_rollout` sizes the buffers with."""
        obs = sum(int(np.prod(self.state_keys[i][2], dtype=np.int64)) * np.dtype(self.state_keys[i][1]).itemsize
                  for i in self.rollout_obs_keys())
        act = int(np.prod(self.action_shape, dtype=np.int64)) * np.dtype(self.action_dtype).itemsize
        return obs, act

    def rollout_begin(self, horizon: int, episodes: int = 0, moments: bool = False) -> None:
        """Opens the pool's rollout collector (RuntimeError("rollout not implemented for this environment") for the
        PGX games; ValueError for an async pool): time-major buffers of `horizon` steps in device memory that
        `rollout_step` fills, `episodes` rows for finished episodes, and with `moments` the float64 power sums of the
        float observation keys.  A pool has one collector; a new one replaces it."""
        if self.players != 1:
            raise RuntimeError("rollout not implemented for this environment")
        if not self._is_sync:
            raise ValueError("rollout: async mode (batch_size != num_envs) is not supported")
        obs, act = self.rollout_row_bytes()
        horizon, episodes, moments = native.check_rollout(horizon, episodes, moments, self.num_envs, obs, act)
        native.check(self._lib.epa_rollout_begin(self._h, horizon, episodes, native.ROLLOUT_MOMENTS if moments else 0))
        self.rollout_horizon, self.rollout_capacity = horizon, episodes

    def rollout_shape(self) -> tuple[int, ...]:
        """(T, N, episodes, t, obs keys, moment components, step counter, flags) of the open collector."""
        out = (ctypes.c_int64 * 8)()
        native.check(self._lib.epa_rollout_shape(self._h, out))
        return tuple(int(x) for x in out)

    def _rollout_host_rows(self) -> tuple[list[np.ndarray], Any]:
        outs = [np.empty((self.num_envs, *shape), dtype=dtype) for _, dtype, shape in self.state_keys]
        return outs, (ctypes.c_void_p * len(outs))(*[o.ctypes.data for o in outs])

    def rollout_reset(self) -> list[np.ndarray]:
        """Resets every env through the collector and returns what `recv` would: the observations also land in slot 0,
        the carried done flags and the episode accumulators are cleared and t = 0."""
        outs, ptrs = self._rollout_host_rows()
        k = ctypes.c_int32(0)
        native.check(self._lib.epa_rollout_reset(self._h, 0, ptrs, len(outs), self.num_envs, ctypes.byref(k)))
        return outs

    def rollout_step(self, action: Any) -> list[np.ndarray]:
        """One step of every env in id order with `action` [N, ...] and the collector's kernels behind it; returns what
        `send` + `recv` return."""
        action = np.ascontiguousarray(action, dtype=self.action_dtype)
        want = (self.num_envs, *self.action_shape)
        if action.size != int(np.prod(want)):
            raise RuntimeError(f"Expected action of shape {want}, got {action.shape}")
        outs, ptrs = self._rollout_host_rows()
        k = ctypes.c_int32(0)
        native.check(self._lib.epa_rollout_step(self._h, action.ctypes.data, ptrs, len(outs), self.num_envs,
                                                ctypes.byref(k)))
        return outs

    def rollout_reset_device(self) -> tuple[list[int], int]:
        """`rollout_reset` on the device path: only enqueued; the device pointers `recv_device` would return."""
        n = len(self.state_keys)
        ptrs = (ctypes.c_void_p * n)()
        k = ctypes.c_int32(0)
        native.check(self._lib.epa_rollout_reset(self._h, 1, ptrs, n, 0, ctypes.byref(k)))
        return [int(p) if p else 0 for p in ptrs], k.value

    def rollout_step_device(self, d_action: int, wait_event: int | None = None) -> tuple[list[int], int]:
        """`rollout_step` with the action rows at the raw device address `d_action`: only enqueued on the pool's
        stream; the device pointers `step_device` would return."""
        n = len(self.state_keys)
        ptrs = (ctypes.c_void_p * n)()
        k = ctypes.c_int32(0)
        native.check(self._lib.epa_rollout_step_device(self._h, ctypes.c_void_p(d_action), ctypes.c_void_p(wait_event),
                                                       ptrs, n, ctypes.byref(k)))
        return [int(p) if p else 0 for p in ptrs], k.value

    def rollout_arrays(self) -> list[tuple[str, Any, tuple[int, ...]]]:
        """(name, dtype, shape) of the collector's buffers in the order of `rollout_view_device`: the obs keys
        [T+1, N, ...], then action [T, N, ...], reward float32, term, trunc, mask uint8 [T, N]."""
        t, n = self.rollout_horizon, self.num_envs
        out = [(self.state_keys[i][0], self.state_keys[i][1], (t + 1, n, *self.state_keys[i][2]))
               for i in self.rollout_obs_keys()]
        out.append(("action", self.action_dtype, (t, n, *self.action_shape)))
        out.append(("reward", np.float32, (t, n)))
        out += [(name, np.uint8, (t, n)) for name in ("term", "trunc", "mask")]
        return out

    def rollout_view_device(self) -> list[int]:
        """The raw device addresses of the buffers, in the order of `rollout_arrays`."""
        n = len(self.rollout_obs_keys()) + 5
        arrays = (ctypes.c_void_p * n)()
        native.check(self._lib.epa_rollout_view_device(self._h, arrays, n))
        return [int(p) for p in arrays]

    def rollout_batch(self) -> dict[str, np.ndarray]:
        """The buffers copied to the host, by the names of `rollout_arrays`, whole: slots beyond t read 0."""
        spec = self.rollout_arrays()
        outs = [np.empty(shape, dtype=dtype) for _, dtype, shape in spec]
        ptrs = (ctypes.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
        native.check(self._lib.epa_rollout_batch(self._h, ptrs, len(outs)))
        return {name: o for (name, _, _), o in zip(spec, outs)}

    def rollout_gae(self, values: Any, gamma: float, lam: float) -> tuple[np.ndarray, np.ndarray]:
        """(advantages, returns) float32 [T, N] of the full horizon from `values` float32 [T+1, N] (rollout.hip.h:
        GaeStep)."""
        t, n = self.rollout_horizon, self.num_envs
        _, _, _, values, gamma, lam = native.check_rollout(t, 0, False, n, values=values, gamma=gamma, lam=lam)
        adv, ret = np.empty((t, n), dtype=np.float32), np.empty((t, n), dtype=np.float32)
        native.check(self._lib.epa_rollout_gae(self._h, values.ctypes.data, gamma, lam, adv.ctypes.data,
                                               ret.ctypes.data))
        return adv, ret

    def rollout_gae_device(self, d_values: int, gamma: float, lam: float, d_adv: int, d_ret: int) -> None:
        """`rollout_gae` on raw device addresses (float32, 4-byte aligned): only enqueued."""
        native.check(self._lib.epa_rollout_gae_device(self._h, ctypes.c_void_p(d_values), float(np.float32(gamma)),
                                                      float(np.float32(lam)), ctypes.c_void_p(d_adv),
                                                      ctypes.c_void_p(d_ret)))

    def rollout_counters(self) -> np.ndarray:
        """int64 [6]: episode rows, episodes finished and dropped since begin, the step counter, t, reset done."""
        out = np.zeros(6, dtype=np.int64)
        native.check(self._lib.epa_rollout_counters(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return out

    def rollout_episodes(self) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """The finished episodes so far -- (env_id int32, step int64, return float64, length int32) in (step, env id)
        order -- and the count back to 0."""
        n = int(self.rollout_counters()[0])
        out = (np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int64), np.empty(n, dtype=np.float64),
               np.empty(n, dtype=np.int32))
        got = ctypes.c_int32(0)
        native.check(self._lib.epa_rollout_episodes(self._h, n, *[o.ctypes.data for o in out], ctypes.byref(got)))
        return out

    def rollout_episodes_view_device(self) -> tuple[list[int], int]:
        """The raw addresses of the four episode arrays (over the capacity) and of the device int32 count."""
        arrays = (ctypes.c_void_p * 4)()
        count = ctypes.c_void_p()
        native.check(self._lib.epa_rollout_episodes_view_device(self._h, arrays, ctypes.byref(count)))
        return [int(p) for p in arrays], int(count.value)

    def rollout_moments(self) -> np.ndarray:
        """float64 [3, components]: count, sum and sum of squares per component of the float obs keys."""
        comps = self.rollout_shape()[5]
        out = np.zeros((3, comps), dtype=np.float64)
        native.check(self._lib.epa_rollout_moments(self._h, out.ctypes.data, None))
        return out

    def rollout_moments_device(self) -> tuple[int, int]:
        """(the raw device address of the [3, components] float64 accumulators, components)."""
        d = ctypes.c_void_p()
        native.check(self._lib.epa_rollout_moments(self._h, None, ctypes.byref(d)))
        return int(d.value), self.rollout_shape()[5]

    def rollout_next(self) -> None:
        """Slot t becomes slot 0 and t = 0; only enqueued."""
        native.check(self._lib.epa_rollout_next(self._h))

    def rollout_end(self) -> None:
        """Closes the collector and releases its device memory; ValueError without one."""
        native.check(self._lib.epa_rollout_end(self._h))

    # -- rollout actor (csrc/actor.hip.h) ----------------------------------------------
    def actor_begin(self, actor: Any, seed: int = 0, deterministic: bool = False, actions: Any = None) -> None:
        """Attaches `actor` (envpool_amd.actor.Actor) to the open collector: ValueError without a collector, for a blob
        of another F, H or kind than the pool's, and when logp and value push the collector past the 2 GiB limit.
        `actions`: the number of actions of the env's Discrete space (the engine knows the action row, not the count;
        default: the actor's own)."""
        if self.players != 1:
            raise RuntimeError("rollout not implemented for this environment")
        if not isinstance(deterministic, (bool, np.bool_)):
            raise ValueError(f"actor: deterministic = {deterministic!r} must be a bool")
        if getattr(self, "rollout_horizon", None) is not None:
            obs, act = self.rollout_row_bytes()
            native.check_rollout(self.rollout_horizon, self.rollout_capacity, False, self.num_envs, obs, act,
                                 actor=True)
        blob = actor.blob()
        low = np.ascontiguousarray(actor.low, np.float64)
        high = np.ascontiguousarray(actor.high, np.float64)
        native.check(self._lib.epa_actor_begin(
            self._h, blob.ctypes.data, blob.nbytes, int(seed) & (2**64 - 1),
            native.ACTOR_DETERMINISTIC if deterministic else 0, int(actor.actions if actions is None else actions),
            low.ctypes.data if actor.kind == 1 else None, high.ctypes.data if actor.kind == 1 else None))

    def actor_shape(self) -> tuple[int, ...]:
        """(F, H, kind, flags) of the attached actor."""
        out = (ctypes.c_int64 * 4)()
        native.check(self._lib.epa_actor_shape(self._h, out))
        return tuple(int(x) for x in out)

    def actor_end(self) -> None:
        native.check(self._lib.epa_actor_end(self._h))

    def actor_eval(self, obs: Any, env_ids: Any, step: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(action, logp, value) of the attached actor on caller rows: `obs` one array per obs key (or the array, for a
        single key) with a row per listed global env id, at the collector step counter `step`.  Nothing of the pool
        changes."""
        keys = self.rollout_obs_keys()
        obs = [obs] if isinstance(obs, np.ndarray) else list(obs)
        ids = np.ascontiguousarray(env_ids, np.int32).reshape(-1)
        if len(obs) != len(keys):
            raise ValueError(f"actor eval: {len(obs)} observation arrays for {len(keys)} obs keys")
        rows = []
        for i, o in zip(keys, obs):
            _, dtype, shape = self.state_keys[i]
            o = np.ascontiguousarray(o, dtype=dtype)
            if o.shape != (len(ids), *shape):
                raise ValueError(f"actor eval: observation of shape {o.shape} for {(len(ids), *shape)}")
            rows.append(o)
        ptrs = (ctypes.c_void_p * len(rows))(*[o.ctypes.data for o in rows])
        action = np.empty((len(ids), *self.action_shape), dtype=self.action_dtype)
        logp, value = np.empty(len(ids), np.float32), np.empty(len(ids), np.float32)
        native.check(self._lib.epa_actor_eval(self._h, ids.ctypes.data, len(ids), int(step), ptrs, len(rows),
                                              action.ctypes.data, logp.ctypes.data, value.ctypes.data))
        return action, logp, value

    def actor_eval_device(self, d_obs: list[int], d_env_ids: int, k: int, step: int, d_action: int, d_logp: int,
                          d_value: int) -> None:
        """`actor_eval` on raw device addresses: only enqueued on the pool's stream."""
        ptrs = (ctypes.c_void_p * len(d_obs))(*d_obs)
        native.check(self._lib.epa_actor_eval_device(self._h, ctypes.c_void_p(d_env_ids), int(k), int(step), ptrs,
                                                     len(d_obs), ctypes.c_void_p(d_action), ctypes.c_void_p(d_logp),
                                                     ctypes.c_void_p(d_value)))

    def actor_view_device(self) -> tuple[int, int]:
        """The raw device addresses of logp float32 [T, N] and value float32 [T + 1, N]."""
        logp, value = ctypes.c_void_p(), ctypes.c_void_p()
        native.check(self._lib.epa_actor_view_device(self._h, ctypes.byref(logp), ctypes.byref(value)))
        return int(logp.value), int(value.value)

    def actor_batch(self) -> tuple[np.ndarray, np.ndarray]:
        """(logp [T, N], value [T + 1, N]) copied to the host, whole."""
        t, n = self.rollout_horizon, self.num_envs
        logp, value = np.empty((t, n), np.float32), np.empty((t + 1, n), np.float32)
        native.check(self._lib.epa_actor_batch(self._h, logp.ctypes.data, value.ctypes.data))
        return logp, value

    def rollout_collect(self, steps: int = 0, wait: bool = True) -> None:
        """`steps` steps of the collector (0: the rest of the horizon) played by the attached actor from C++: features,
        net, sample, step, store, scan, moments per step, then the value of slot t.  `wait=False` only enqueues."""
        if isinstance(steps, (bool, np.bool_)) or not isinstance(steps, (int, np.integer)) or int(steps) < 0:
            raise ValueError(f"rollout collect: steps = {steps!r} must be an integer of at least 0")
        fn = self._lib.epa_rollout_collect if wait else self._lib.epa_rollout_collect_device
        native.check(fn(self._h, int(steps)))

    def rollout_gae_stored(self, gamma: float, lam: float) -> tuple[np.ndarray, np.ndarray]:
        """`rollout_gae` with the values the attached actor stored."""
        t, n = self.rollout_horizon, self.num_envs
        # (gae's checks of gamma and lam; the values are the device's own)
        _, _, _, _, gamma, lam = native.check_rollout(1, 0, False, 1, values=np.zeros((2, 1), np.float32),
                                                      gamma=gamma, lam=lam)
        adv, ret = np.empty((t, n), dtype=np.float32), np.empty((t, n), dtype=np.float32)
        native.check(self._lib.epa_rollout_gae(self._h, None, gamma, lam, adv.ctypes.data, ret.ctypes.data))
        return adv, ret

    # -- self-play driver (csrc/pgx_selfplay.hip.h) -----------------------------------
    def selfplay_begin(self, net: Any, **options: Any) -> None:
        """Opens the pool's self-play driver (epa_selfplay_begin) with the built-in network `net` as the evaluator;
        `options` are `native.check_selfplay`'s.  A pool has one driver; a new one replaces it.  It needs a pool in
        sync mode with nothing pending in its result queue, and with `record` an open recorder."""
        o, x = native.check_selfplay(**options), native.selfplay_extra_of(options)
        self.guided_shape()
        native.check(self._lib.epa_selfplay_begin_ex(self._h, net._handle(self.device), None, ctypes.byref(o),
                                                     ctypes.byref(x)))
        self._selfplay_net = net  # (the driver uses the net's device copy: it must live as long)

    def selfplay_run(self, plies: int, wait: bool = True) -> None:
        """Plays `plies` plies of every env (epa_selfplay_run); `wait=False` only enqueues them on the pool's stream
        (epa_selfplay_run_device).  The driver opens the pool's guided-search session ply by ply: a session the caller
        had open is gone afterwards."""
        plies = native.check_selfplay_plies(plies)
        run = self._lib.epa_selfplay_run if wait else self._lib.epa_selfplay_run_device
        self._guided_k = None
        native.check(run(self._h, plies))

    def selfplay_stats(self) -> np.ndarray:
        """int64 [6]: games, wins0, wins1, draws, plies, t since the driver was opened; waits for the device."""
        out = np.zeros(6, dtype=np.int64)
        native.check(self._lib.epa_selfplay_stats(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return out

    def selfplay_end(self) -> None:
        """Closes the driver and releases its device memory; ValueError without one.  The recorder stays open."""
        native.check(self._lib.epa_selfplay_end(self._h))
        self._selfplay_net = None

    def selfplay_noise(self) -> np.ndarray:
        """float32 [num_envs, A]: the host copy of the last ply's noise rows (epa_selfplay_noise) -- the Dirichlet eta
        of a PUCT driver (zeros without `dirichlet_alpha`, and before the first ply), the Gumbel rows of a Gumbel
        driver; waits for the device."""
        out = np.zeros((self.num_envs, self.guided_shape()[3]), dtype=np.float32)
        native.check(self._lib.epa_selfplay_noise(self._h, ctypes.c_void_p(out.ctypes.data)))
        return out

    # -- arena (csrc/pgx_arena.hip.h) ---------------------------------------------------
    def net_eval_pair(self, net_a: Any, net_b: Any, obs: Any, mask: Any, status: Any, side: Any,
                      priors: bool = False) -> tuple[np.ndarray, np.ndarray]:
        """`net_eval` with two networks (epa_net_eval_pair): row r is evaluated by `net_a` where `side[r]` is 0 and
        by `net_b` where it is 1, grouped by net on the device and evaluated in one launch.  Every row gets exactly
        what `net_eval` of its net gives it."""
        native.check_arena(net_a, net_b)
        obs, mask, status = self._net_rows("net_eval_pair", obs, mask, status)
        side = native.check_arena_side(side, len(status))
        a = self.guided_shape()[3]
        policy, value = np.empty((len(status), a), dtype=np.float32), np.empty(len(status), dtype=np.float32)
        native.check(self._lib.epa_net_eval_pair(
            self._h, net_a._handle(self.device), net_b._handle(self.device), len(status), 1 if priors else 0,
            obs.ctypes.data, mask.ctypes.data, status.ctypes.data, side.ctypes.data, policy.ctypes.data,
            value.ctypes.data))
        return policy, value

    def net_eval_pair_device(self, net_a: Any, net_b: Any, rows: int, priors: bool, d_obs: int, d_mask: int,
                             d_status: int, d_side: int, d_policy: int, d_value: int) -> None:
        """`net_eval_pair` on device memory at raw addresses (policy and value 4-byte aligned; a side byte that is not
        0 counts as 1): only enqueued on the pool's stream."""
        native.check_arena(net_a, net_b)
        self.guided_shape()
        native.check(self._lib.epa_net_eval_pair_device(
            self._h, net_a._handle(self.device), net_b._handle(self.device), int(rows), 1 if priors else 0,
            ctypes.c_void_p(d_obs), ctypes.c_void_p(d_mask), ctypes.c_void_p(d_status), ctypes.c_void_p(d_side),
            ctypes.c_void_p(d_policy), ctypes.c_void_p(d_value)))

    def arena_begin(self, net_a: Any, net_b: Any, **options: Any) -> None:
        """Opens the pool's driver as an arena (epa_arena_begin): `net_a` moves for seat (e & 1) of the env with global
        id e and `net_b` for the other seat.  `options` are `native.check_arena`'s: `selfplay_begin`'s, with `record`
        False by default.  `selfplay_run` and `selfplay_end` drive and close it."""
        o, x = native.check_arena(net_a, net_b, **options), native.selfplay_extra_of(options)
        self.guided_shape()
        native.check(self._lib.epa_selfplay_begin_ex(self._h, net_a._handle(self.device), net_b._handle(self.device),
                                                     ctypes.byref(o), ctypes.byref(x)))
        self._selfplay_net = (net_a, net_b)  # (the driver uses the nets' device copies: they must live as long)

    def arena_run(self, plies: int, wait: bool = True) -> None:
        """`selfplay_run` of an arena."""
        self.selfplay_run(plies, wait)

    def arena_stats(self) -> np.ndarray:
        """int64 [8]: games, wins0, wins1, draws, plies, wins_a, wins_b, t since the arena was opened; waits for the
        device.  ValueError on a driver that is no arena."""
        out = np.zeros(8, dtype=np.int64)
        native.check(self._lib.epa_arena_stats(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return out

    def arena_end(self) -> None:
        """`selfplay_end` of an arena."""
        self.selfplay_end()

    def _ids(self, env_ids: Any) -> np.ndarray:
        if env_ids is None:
            return np.arange(
                self.env_id_offset, self.env_id_offset + self.num_envs, dtype=np.int32
            )
        return np.ascontiguousarray(env_ids, dtype=np.int32)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.epa_destroy(self._h)
            self._h = None
        if getattr(self, "_blocks", None) is not None:
            self._blocks.close()  # blocks still lent out are freed when their arrays die

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:
            pass
