"""Native (spec, pool) class pairs for the Python adaptors.

In the reference these classes come out of the pybind11 `REGISTER` macro
(envpool/core/py_envpool.h:303-332): `_XxxEnvSpec` exposing
`_config_keys/_default_config_values/_state_keys/_action_keys/_config_values/
_state_spec/_action_spec`, and `_XxxEnvPool` exposing
`_spec/_send/_recv/_reset/_render/_xla`.  Here the same surface is produced by
`make_native_classes(FamilyDef)` on top of the C ABI (core/native.py), so the
adaptors under envpool_amd/python are oblivious to the swap.

Spec tuples follow SpecTupleHelper (py_envpool.h:103-110):
  (np.dtype, shape list, (lo, hi), (elementwise lo[], hi[]), is_discrete)
with the reference's defaults for unbounded specs, i.e.
std::numeric_limits<T>::min()/max() (envpool/core/spec.h:71-72; note that
::min() of a float type is the smallest positive normal, as in the reference).
"""

from __future__ import annotations

import collections
import ctypes
import threading
from dataclasses import dataclass, field
from typing import Any, Callable, Sequence

import numpy as np

from .. import sharding
from . import native
from .device_pool import DevicePool

INT_MAX = 2**31 - 1
INT_MIN = -(2**31)
F32_MIN, F32_MAX = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
F64_MIN, F64_MAX = float(np.finfo(np.float64).tiny), float(np.finfo(np.float64).max)

_DEFAULT_BOUNDS = {
    np.dtype(np.int32): (INT_MIN, INT_MAX),
    np.dtype(np.float32): (F32_MIN, F32_MAX),
    np.dtype(np.float64): (F64_MIN, F64_MAX),
    np.dtype(np.bool_): (False, True),
    np.dtype(np.uint8): (0, 255),
    np.dtype(np.int8): (-128, 127),
}


def spec(dtype: Any, shape: Sequence[int], bounds: tuple | None = None,
         elementwise: tuple | None = None, is_discrete: bool = False) -> tuple:
    dt = np.dtype(dtype)
    if bounds is None:
        bounds = _DEFAULT_BOUNDS[dt]
    if elementwise is None:
        elementwise = ([], [])
    return (dt, list(shape), tuple(bounds), (list(elementwise[0]), list(elementwise[1])),
            bool(is_discrete))


# common_config / common_action_spec / common_state_spec: env_spec.h:26-43
COMMON_CONFIG: list[tuple[str, Any]] = [
    ("num_envs", 1),
    ("batch_size", 0),
    ("num_threads", 0),
    ("max_num_players", 1),
    ("thread_affinity_offset", -1),
    ("base_path", "envpool"),
    ("seed", 42),
    ("env_seed", []),
    ("gym_reset_return_info", True),
    ("max_episode_steps", INT_MAX),
]
# extensions of this engine, appended AFTER the env-specific keys so that the
# reference's prefix of config keys is unchanged
EXTENSION_CONFIG: list[tuple[str, Any]] = [
    ("device", 0),          # HIP device ordinal, or a list of ordinals to shard over
    ("env_id_offset", 0),   # global id of local env 0 (one shard of a bigger pool)
    # how long recv() waits for rows nobody has sent yet: -1 forever, like the reference's blocking Recv
    # (async_envpool.h:169-181), 0 raise RuntimeError at once, > 0 raise after that many milliseconds
    ("recv_timeout_ms", -1),
]
COMMON_ACTION_SPEC = [
    ("env_id", spec(np.int32, [])),
    ("players.env_id", spec(np.int32, [-1])),
]
COMMON_STATE_SPEC = [
    ("info:env_id", spec(np.int32, [])),
    ("info:players.env_id", spec(np.int32, [-1])),
    ("elapsed_step", spec(np.int32, [])),
    ("done", spec(np.bool_, [])),
    ("reward", spec(np.float32, [-1])),
    ("discount", spec(np.float32, [-1], (0.0, 1.0))),
    ("step_type", spec(np.int32, [])),
    ("trunc", spec(np.bool_, [])),
]


@dataclass
class FamilyDef:
    """Python-side description of `XxxEnvFns` of the reference."""

    name: str                       # class stem, e.g. "CartPole" / "GymHalfCheetah"
    native: str                     # family name understood by the C ABI
    default_config: list[tuple[str, Any]]
    state_spec: Callable[[dict], list[tuple[str, tuple]]]
    action_spec: Callable[[dict], list[tuple[str, tuple]]]
    # config -> numeric params forwarded to the C ABI (epa_config.param_*)
    native_params: Callable[[dict], dict[str, float]] = lambda conf: {}
    # config keys accepted for API compatibility but not supported when changed
    unsupported: dict[str, Any] = field(default_factory=dict)
    # (conf, DevicePool kwargs) -> pool, for families with their own constructor (Atari)
    pool_factory: Callable[[dict, dict], Any] | None = None
    # players per env (the PGX board games: 2); max_num_players must equal it
    players: int = 1


class _ShardedPools:
    """num_envs split contiguously over several GPUs of one process:
    shard s owns env ids [offset + s*per, offset + (s+1)*per).  Each shard is a
    DevicePool with its own streams and its own host thread, so uploads, step
    kernels and downloads of all GPUs run concurrently; there is no inter-GPU
    traffic on the data path ("host gather").

    recv: every shard copies its rows device->host DIRECTLY into its row range of
    ONE pinned block (epa_recv_into) whenever the batch is grouped by shard (the
    `step(action)` / `reset()` case, ids ascending) -- no host-side scatter.  Only
    batches whose ids interleave shards fall back to a per-shard recv + scatter."""

    def __init__(self, family: str, devices: Sequence[int], num_envs: int, **kw: Any):
        import concurrent.futures

        if num_envs % len(devices) != 0:
            raise ValueError("num_envs must be divisible by the number of devices")
        if kw.get("batch_size", 0) not in (0, num_envs):
            raise ValueError("async mode (batch_size < num_envs) needs a single device")
        self.per = num_envs // len(devices)
        self.offset = kw.pop("env_id_offset", 0)
        env_seed = kw.pop("env_seed", None)
        kw.pop("batch_size", None)
        self.pools = [
            DevicePool(family, self.per, device=d, env_id_offset=self.offset + s * self.per,
                       env_seed=(env_seed[s * self.per:(s + 1) * self.per] if env_seed else None),
                       **kw)
            for s, d in enumerate(devices)
        ]
        self.state_keys = self.pools[0].state_keys
        self._pending: collections.deque = collections.deque()
        # recv() blocks until a send / reset has been split over the shards (a consumer thread may arrive first)
        self._cv = threading.Condition()
        self._timeout_ms = float((kw.get("params") or {}).get("recv_timeout_ms", -1))
        # one host thread per GPU: the C ABI calls release the GIL (ctypes)
        self._exec = concurrent.futures.ThreadPoolExecutor(len(self.pools))
        self._blocks = self.pools[0]._blocks
        self._lib = self.pools[0]._lib

    def _split(self, ids: np.ndarray) -> tuple[list[Any], bool]:
        """Rows of each shard; `grouped` when every shard's rows are one contiguous run
        (then parts are slices)."""
        shard = (ids - self.offset) // self.per
        if len(ids) and np.all(shard[1:] >= shard[:-1]):
            bounds = np.searchsorted(shard, np.arange(len(self.pools) + 1))
            return [slice(int(bounds[s]), int(bounds[s + 1])) for s in range(len(self.pools))], True
        return [np.flatnonzero(shard == s) for s in range(len(self.pools))], False

    @staticmethod
    def _count(part: Any) -> int:
        return part.stop - part.start if isinstance(part, slice) else len(part)

    def _each(self, fn: Callable[[int, DevicePool, Any], Any], parts: list[Any]) -> None:
        futs = [self._exec.submit(fn, s, p, part)
                for s, (p, part) in enumerate(zip(self.pools, parts)) if self._count(part)]
        for f in futs:
            f.result()

    def send(self, env_id: np.ndarray, action: np.ndarray) -> None:
        env_id = np.ascontiguousarray(env_id, dtype=np.int32)
        action = np.asarray(action)
        parts, grouped = self._split(env_id)
        # (a shard's rows land in ITS row range of one block shared by all shards, epa_recv_into: no block to post)
        self._each(lambda s, p, part: p.send(env_id[part], action[part], post_block=False), parts)
        with self._cv:
            self._pending.append((len(env_id), parts, grouped))
            self._cv.notify_all()

    def reset(self, env_ids: np.ndarray) -> None:
        env_ids = np.ascontiguousarray(env_ids, dtype=np.int32)
        parts, grouped = self._split(env_ids)
        self._each(lambda s, p, part: p.reset(env_ids[part]), parts)
        with self._cv:
            self._pending.append((len(env_ids), parts, grouped))
            self._cv.notify_all()

    def recv(self) -> list[np.ndarray]:
        with self._cv:
            timeout = None if self._timeout_ms < 0 else self._timeout_ms / 1000.0
            if not self._cv.wait_for(lambda: bool(self._pending), timeout):
                raise RuntimeError(f"recv: nothing pending (recv_timeout_ms = {self._timeout_ms:g})")
            k, parts, grouped = self._pending.popleft()
        if not grouped:
            outs = [np.empty((k, *shape), dtype=dtype) for _, dtype, shape in self.state_keys]

            def scatter(s: int, p: DevicePool, idx: Any) -> None:
                for o, part in zip(outs, p.recv()):
                    o[idx] = part.reshape((-1, *o.shape[1:]))  # (a per-player key: back to one row per env)

            self._each(scatter, parts)
            return self.pools[0].player_rows(outs)
        # one pinned block for the whole batch, laid out like a DevicePool batch of k rows
        row_bytes = [int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
                     for _, dtype, shape in self.state_keys]
        offs, total = [], 0
        for rb in row_bytes:
            offs.append(total)
            total += (k * rb + 255) // 256 * 256
        block = self._blocks.take(max(total, 256))
        base = block.ctypes.data
        n = len(self.state_keys)

        def land(s: int, p: DevicePool, part: slice) -> None:
            ptrs = (ctypes.c_void_p * n)(*[base + o + part.start * rb
                                           for o, rb in zip(offs, row_bytes)])
            got = ctypes.c_int32(0)
            native.check(self._lib.epa_recv_into(p._h, ptrs, n, part.stop - part.start,
                                                 ctypes.byref(got)))
            assert got.value == part.stop - part.start
            p.pop_pending()

        self._each(land, parts)
        return self.pools[0].player_rows([block[o:o + k * rb].view(dtype).reshape((k, *shape))
                                          for (_, dtype, shape), o, rb in zip(self.state_keys, offs, row_bytes)])

    def render_size(self, width: int = 0, height: int = 0) -> tuple[int, int]:
        return self.pools[0].render_size(width, height)

    def render(self, env_ids: Any, width: int = 0, height: int = 0, camera_id: int = -1) -> np.ndarray:
        """Frames of envs of any shards, in request order: every shard renders its ids, all shards at once."""
        ids = np.ascontiguousarray(env_ids, dtype=np.int32).reshape(-1)
        w, h = self.render_size(width, height)
        if len(ids) == 0:
            raise ValueError("render env_ids must not be empty")
        shard = (ids - self.offset) // self.per
        bad = ids[(shard < 0) | (shard >= len(self.pools))]
        if len(bad):
            raise ValueError(f"env_id {int(bad[0])} out of range")
        out = np.empty((len(ids), h, w, 3), dtype=np.uint8)

        def paint(s: int, p: DevicePool, idx: Any) -> None:
            out[idx] = p.render(ids[idx], width, height, camera_id)

        self._each(paint, [np.flatnonzero(shard == s) for s in range(len(self.pools))])
        return out

    def snapshot(self, env_ids: Any = None, rng: bool = True) -> list[np.ndarray]:
        """One blob per shard, all shards at once; only of the whole pool."""
        if env_ids is not None:
            raise ValueError("snapshot of a sharded pool takes no env_ids: it is one blob per shard")
        blobs: list[Any] = [None] * len(self.pools)

        def take(s: int, p: DevicePool, _: Any) -> None:
            blobs[s] = p.snapshot(None, rng)

        self._each(take, [slice(0, self.per)] * len(self.pools))
        return blobs

    def restore(self, blobs: Any, env_ids: Any = None) -> None:
        """The list `snapshot` returned (of this pool or of one sharded the same way), shard by shard."""
        if env_ids is not None:
            raise ValueError("restore of a sharded pool takes no env_ids: it is one blob per shard")
        if not isinstance(blobs, (list, tuple)) or len(blobs) != len(self.pools):
            raise ValueError(f"restore of a sharded pool takes a list of {len(self.pools)} blobs, one per shard")
        for b in blobs:
            if native.snapshot_header(np.ascontiguousarray(b))[0] != self.per:
                raise ValueError(f"restore of a sharded pool: every blob must hold the {self.per} envs of its shard")
        self._each(lambda s, p, _: p.restore(blobs[s], None), [slice(0, self.per)] * len(self.pools))

    def fork(self, src: Any, dst: Any, rng: bool = True) -> None:
        """Within shards only: a pair whose envs live on different devices is refused."""
        src = np.ascontiguousarray(src, dtype=np.int32).reshape(-1)
        dst = np.ascontiguousarray(dst, dtype=np.int32).reshape(-1)
        if len(src) != len(dst):
            raise ValueError(f"fork: {len(src)} source ids for {len(dst)} targets")
        parts = sharding.fork_parts(src, dst, self.offset, self.per, len(self.pools))
        self._each(lambda s, p, idx: p.fork(src[idx], dst[idx], rng), parts)

    def playout(self, env_ids: Any = None, repeats: int = 1, max_plies: int = 0, seed: int = 0,
                commit: bool = False) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Playouts of envs of any shards, rows in request order: every shard plays its ids, all shards at once.
        The draws are keyed by the global env id, so the rows are those of the unsharded pool."""
        if env_ids is None:
            env_ids = np.arange(self.offset, self.offset + self.per * len(self.pools), dtype=np.int32)
        ids = native.check_playout(env_ids, repeats, max_plies, commit)
        shard = (ids - self.offset) // self.per
        bad = ids[(shard < 0) | (shard >= len(self.pools))]
        if len(bad):
            raise ValueError(f"env_id {int(bad[0])} out of range")
        k, r = len(ids), int(repeats)
        returns = np.empty((k, r, 2), dtype=np.float32)
        plies = np.empty((k, r), dtype=np.int32)
        status = np.empty((k, r), dtype=np.uint8)

        def play(s: int, p: DevicePool, idx: Any) -> None:
            returns[idx], plies[idx], status[idx] = p.playout(ids[idx], repeats, max_plies, seed, commit)

        self._each(play, [np.flatnonzero(shard == s) for s in range(len(self.pools))])
        return returns, plies, status

    def search(self, env_ids: Any = None, simulations: int = 64, leaf_playouts: int = 8, c_puct: float = 1.25,
               max_plies: int = 0, seed: int = 0) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Searches from envs of any shards, rows in request order: every shard searches its ids, all shards at once.
        The leaf playouts are keyed by the global env id, so the rows are those of the unsharded pool."""
        if env_ids is None:
            env_ids = np.arange(self.offset, self.offset + self.per * len(self.pools), dtype=np.int32)
        ids = native.check_search(env_ids, simulations, leaf_playouts, c_puct, max_plies)
        shard = (ids - self.offset) // self.per
        bad = ids[(shard < 0) | (shard >= len(self.pools))]
        if len(bad):
            raise ValueError(f"env_id {int(bad[0])} out of range")
        k, a = len(ids), self.pools[0].search_actions()
        visits = np.empty((k, a), dtype=np.int32)
        returns = np.empty((k, a), dtype=np.int32)
        action = np.empty(k, dtype=np.int32)

        def run(s: int, p: DevicePool, idx: Any) -> None:
            visits[idx], returns[idx], action[idx] = p.search(ids[idx], simulations, leaf_playouts, c_puct,
                                                              max_plies, seed)

        self._each(run, [np.flatnonzero(shard == s) for s in range(len(self.pools))])
        return visits, returns, action

    def solve(self, env_ids: Any = None, depth: int = 0, max_nodes: int = 1 << 20,
              table_bits: int = 0) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """Solves envs of any shards, rows in request order: every shard solves its ids, all shards at once.  A row
        depends on its position, depth, max_nodes and table_bits only (a table is private to a lane of the row's
        wave), so the rows are those of the unsharded pool."""
        if env_ids is None:
            env_ids = np.arange(self.offset, self.offset + self.per * len(self.pools), dtype=np.int32)
        ids = native.check_solve(env_ids, depth, max_nodes, table_bits)
        shard = (ids - self.offset) // self.per
        bad = ids[(shard < 0) | (shard >= len(self.pools))]
        if len(bad):
            raise ValueError(f"env_id {int(bad[0])} out of range")
        k, a = len(ids), self.pools[0].solve_actions()
        out = (np.empty(k, dtype=np.int8), np.empty((k, a), dtype=np.int8), np.empty(k, dtype=np.int32),
               np.empty(k, dtype=np.uint8), np.empty(k, dtype=np.int64))

        def run(s: int, p: DevicePool, idx: Any) -> None:
            for whole, part in zip(out, p.solve(ids[idx], depth, max_nodes, table_bits)):
                whole[idx] = part

        self._each(run, [np.flatnonzero(shard == s) for s in range(len(self.pools))])
        return out

    # -- guided tree search: one session per shard, rows in request order (host forms only) --
    def guided_shape(self) -> tuple[int, int, int, int]:
        return self.pools[0].guided_shape()

    def _guided_empty(self, k: int, width: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        h, w, c, a = self.guided_shape()
        lead = (k, width) if width else (k,)  # (a wide session's leaves carry the slot axis)
        return (np.empty(lead + (h, w, c), dtype=np.bool_), np.empty(lead + (a,), dtype=np.bool_),
                np.empty(lead, dtype=np.uint8))

    def guided_begin(self, env_ids: Any = None, simulations: int = 64, c_puct: float = 1.25,
                     nodes: int = 0, width: Any = None, tactics: int = 0,
                     tactics_nodes: int = native.GUIDED_TACTICS_NODES,
                     prove: bool = False) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """A session in every shard that owns listed envs, all shards at once.  The search has no random numbers and
        no dependence on the env id, so the rows are those of the unsharded pool.  `width`: a wide session in every
        shard (`DevicePool.guided_begin`).  `tactics`, `tactics_nodes`: the exact leaf status in every shard; what it
        decides depends on the leaf's position alone, so the rows stay those of the unsharded pool.  `prove`: proven
        values in every shard; a proof depends on the root's own tree alone."""
        if env_ids is None:
            env_ids = np.arange(self.offset, self.offset + self.per * len(self.pools), dtype=np.int32)
        ids = native.check_guided(env_ids, simulations, c_puct)
        cap = native.check_guided_nodes(simulations, nodes)
        width = native.check_guided_width(width)
        tactics, tactics_nodes = native.check_guided_tactics(tactics, tactics_nodes)
        prove = native.check_guided_prove(prove)
        h, w, c, a = self.guided_shape()
        shard = (ids - self.offset) // self.per
        bad = ids[(shard < 0) | (shard >= len(self.pools))]
        if len(bad):
            raise ValueError(f"env_id {int(bad[0])} out of range")
        parts = [np.flatnonzero(shard == s) for s in range(len(self.pools))]
        k = len(ids)
        leaves = self._guided_empty(k, width)
        extra = (int(nodes or 0), width) if width else ((nodes,) if nodes else ())
        if tactics:
            extra = (int(nodes or 0), width or None, tactics, tactics_nodes)
        if prove:
            extra = (int(nodes or 0), width or None, tactics, tactics_nodes, True)

        def begin(s: int, p: DevicePool, idx: Any) -> None:
            for o, part in zip(leaves, p.guided_begin(ids[idx], simulations, c_puct, *extra)):
                o[idx] = part

        self._each(begin, parts)
        self._guided = (k, a, parts)
        self._guided_nodes = cap
        self._guided_width = width
        return leaves

    def guided_reroot(self, actions: Any, simulations: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """`guided_reroot` of every shard's session, all shards at once; row i of `actions` goes with root i."""
        k, a, parts = self._guided_session("guided_reroot")
        if getattr(self, "_guided_nodes", None) is None:
            raise ValueError("guided_reroot: reroot not implemented for gumbel sessions")
        actions = native.check_guided_reroot(actions, k, a, simulations, self._guided_nodes)
        leaves = self._guided_empty(k, getattr(self, "_guided_width", 0))

        def reroot(s: int, p: DevicePool, idx: Any) -> None:
            for o, part in zip(leaves, p.guided_reroot(actions[idx], simulations)):
                o[idx] = part

        self._each(reroot, parts)
        return leaves

    def _guided_session(self, what: str) -> tuple:
        g = getattr(self, "_guided", None)
        if g is None:
            raise ValueError(f"{what}: the pool has no guided-search session")
        return g

    def guided_advance(self, priors: Any, values: Any) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        k, a, parts = self._guided_session("guided_advance")
        width = getattr(self, "_guided_width", 0)
        if width:  # the rows of root i are rows i W .. i W + W - 1: split by root
            priors, values = native.check_guided_wide_rows(priors, values, k, width, a)
            priors, values = priors.reshape(k, width, a), values.reshape(k, width)
        else:
            priors, values = native.check_guided_rows(priors, values, k, a)
        leaves = self._guided_empty(k, width)

        def advance(s: int, p: DevicePool, idx: Any) -> None:
            for o, part in zip(leaves, p.guided_advance(priors[idx], values[idx])):
                o[idx] = part

        self._each(advance, parts)
        return leaves

    def guided_result(self) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        k, a, parts = self._guided_session("guided_result")
        out = (np.empty((k, a), dtype=np.int32), np.empty((k, a), dtype=np.float32), np.empty(k, dtype=np.int32))

        def result(s: int, p: DevicePool, idx: Any) -> None:
            for o, part in zip(out, p.guided_result()):
                o[idx] = part

        self._each(result, parts)
        return out

    def guided_decided(self, with_nodes: bool = False) -> Any:
        k, a, parts = self._guided_session("guided_decided")
        out = (np.empty(k, dtype=np.int32), np.empty(k, dtype=np.int64))

        def decided(s: int, p: DevicePool, idx: Any) -> None:
            for o, part in zip(out, p.guided_decided(with_nodes=True)):
                o[idx] = part

        self._each(decided, parts)
        return out if with_nodes else out[0]

    def guided_proof(self) -> tuple[np.ndarray, np.ndarray]:
        k, a, parts = self._guided_session("guided_proof")
        out = (np.empty(k, dtype=np.int8), np.empty((k, a), dtype=np.int8))

        def proof(s: int, p: DevicePool, idx: Any) -> None:
            for o, part in zip(out, p.guided_proof()):
                o[idx] = part

        self._each(proof, parts)
        return out

    def guided_end(self) -> None:
        _, _, parts = self._guided_session("guided_end")
        self._each(lambda s, p, idx: p.guided_end(), parts)
        self._guided = None

    def net_run(self, net: Any, leaves: tuple, advances: Any = None) -> tuple[tuple, int]:
        """`DevicePool.net_run` in every shard that has rows of the session, all shards at once, each with the net's
        copy on its own device; a shard's round ends when its own rows are complete, which changes no row.  Returns
        (the new leaves, the most advances a shard made)."""
        _, _, parts = self._guided_session("net_run")
        advances = native.check_net_advances(advances) or None
        out = tuple(np.array(x) for x in leaves)
        made = [0] * len(self.pools)
        # a net has one copy per device, and calls that use one copy must not overlap: shards that share a device
        # take turns, shards on different devices run at once
        turn = {p.device: threading.Lock() for p in self.pools}

        def run(s: int, p: DevicePool, idx: Any) -> None:
            with turn[p.device]:
                new, made[s] = p.net_run(net, tuple(np.asarray(x)[idx] for x in leaves), advances)
            for o, part in zip(out, new):
                o[idx] = part

        self._each(run, parts)
        return out, max(made)

    def net_eval(self, net: Any, obs: Any, mask: Any, status: Any, priors: bool = False) -> tuple:
        """`DevicePool.net_eval` on the first shard: the rows are positions, whichever shard holds their envs."""
        return self.pools[0].net_eval(net, obs, mask, status, priors)

    # -- Gumbel search: the same sessions with the Gumbel policy; the noise rows follow their ids --
    def gumbel_actions(self) -> int:
        return self.pools[0].gumbel_actions()

    def gumbel_begin(self, gumbel: Any, env_ids: Any = None, simulations: int = 32, max_considered: int = 16,
                     c_visit: float = 50.0, c_scale: float = 0.1,
                     batch: Any = None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """A Gumbel session in every shard that owns listed envs, all shards at once; row i of `gumbel` goes with
        env_ids[i].  The search depends on the positions and the caller's numbers only, so the rows are those of the
        unsharded pool.  `batch`: a batch session in every shard (`DevicePool.gumbel_begin`)."""
        if env_ids is None:
            env_ids = np.arange(self.offset, self.offset + self.per * len(self.pools), dtype=np.int32)
        ids = native.check_gumbel(env_ids, simulations, max_considered, c_visit, c_scale)
        batch = native.check_gumbel_batch(batch)
        self.gumbel_actions()
        h, w, c, a = self.guided_shape()
        gumbel = native.check_gumbel_noise(gumbel, len(ids), a)
        shard = (ids - self.offset) // self.per
        bad = ids[(shard < 0) | (shard >= len(self.pools))]
        if len(bad):
            raise ValueError(f"env_id {int(bad[0])} out of range")
        parts = [np.flatnonzero(shard == s) for s in range(len(self.pools))]
        k = len(ids)
        leaves = self._guided_empty(k, batch)

        def begin(s: int, p: DevicePool, idx: Any) -> None:
            for o, part in zip(leaves, p.gumbel_begin(gumbel[idx], ids[idx], simulations, max_considered, c_visit,
                                                      c_scale, batch or None)):
                o[idx] = part

        self._each(begin, parts)
        self._guided = (k, a, parts)
        self._guided_nodes = None  # (no reroot of a Gumbel session)
        self._gumbel_batch = batch
        return leaves

    def gumbel_advance(self, logits: Any, values: Any) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        k, a, parts = self._guided_session("gumbel_advance")
        batch = getattr(self, "_gumbel_batch", 0)
        if batch:  # the rows of root i are rows i B .. i B + B - 1: split by root
            logits, values = native.check_gumbel_batch_rows(logits, values, k, batch, a)
            logits, values = logits.reshape(k, batch, a), values.reshape(k, batch)
        else:
            logits, values = native.check_gumbel_rows(logits, values, k, a)
        leaves = self._guided_empty(k, batch)

        def advance(s: int, p: DevicePool, idx: Any) -> None:
            for o, part in zip(leaves, p.gumbel_advance(logits[idx], values[idx])):
                o[idx] = part

        self._each(advance, parts)
        return leaves

    def gumbel_result(self) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        k, a, parts = self._guided_session("gumbel_result")
        out = (np.empty((k, a), dtype=np.int32), np.empty((k, a), dtype=np.float32), np.empty(k, dtype=np.int32),
               np.empty((k, a), dtype=np.float32))

        def result(s: int, p: DevicePool, idx: Any) -> None:
            for o, part in zip(out, p.gumbel_result()):
                o[idx] = part

        self._each(result, parts)
        return out

    # -- self-play recorder: one recorder per shard, each of the full capacity (host forms only) --
    def _record_all(self, fn: Callable[[DevicePool], Any]) -> list:
        out: list[Any] = [None] * len(self.pools)

        def run(s: int, p: DevicePool, _: Any) -> None:
            out[s] = fn(p)

        self._each(run, [slice(0, self.per)] * len(self.pools))
        return out

    def _record_parts(self, what: str, env_ids: Any) -> tuple[np.ndarray, list]:
        if env_ids is None:
            env_ids = np.arange(self.offset, self.offset + self.per * len(self.pools), dtype=np.int32)
        ids = native.check_record_ids(what, env_ids)
        shard = (ids - self.offset) // self.per
        bad = ids[(shard < 0) | (shard >= len(self.pools))]
        if len(bad):
            raise ValueError(f"env_id {int(bad[0])} out of range")
        return ids, [np.flatnonzero(shard == s) for s in range(len(self.pools))]

    def record_begin(self, capacity: int, max_plies: int = 0, symmetries: bool = False) -> tuple:
        native.check_record(capacity, max_plies, symmetries)
        return self._record_all(lambda p: p.record_begin(capacity, max_plies, symmetries))[0]

    def record_shape(self) -> tuple:
        return self.pools[0].record_shape()

    def record_add(self, policy: Any, env_ids: Any = None) -> None:
        """Every shard stages its ids, all shards at once; row i of `policy` goes with env_ids[i]."""
        ids, parts = self._record_parts("recorder add", env_ids)
        policy = native.check_record_add(policy, len(ids), self.record_shape()[3])
        self._each(lambda s, p, idx: p.record_add(policy[idx], ids[idx]), parts)

    def record_finish(self, reward: Any, done: Any, env_ids: Any = None) -> None:
        """Every shard finishes its ids in the call's row order, all shards at once."""
        ids, parts = self._record_parts("recorder finish", env_ids)
        reward, done = native.check_record_finish(reward, done, len(ids))
        self._each(lambda s, p, idx: p.record_finish(reward[idx], done[idx], ids[idx]), parts)

    def record_counters(self) -> np.ndarray:
        return np.sum(self._record_all(lambda p: p.record_counters()), axis=0)

    def record_drain(self) -> tuple:
        """The shards' samples behind each other in shard order: while nothing is dropped and the rows of a finish
        are in id order, the unsharded pool's order."""
        parts = self._record_all(lambda p: p.record_drain())
        return tuple(np.concatenate(cols) for cols in zip(*parts))

    def record_discard(self, env_ids: Any = None) -> None:
        if env_ids is None:
            self._record_all(lambda p: p.record_discard(None))
            return
        ids, parts = self._record_parts("recorder discard", env_ids)
        self._each(lambda s, p, idx: p.record_discard(ids[idx]), parts)

    def record_end(self) -> None:
        self._record_all(lambda p: p.record_end())

    # -- rollout collector: one collector per shard, each with the full episode capacity (host forms only).  The
    # shards' arrays are concatenated along N, episodes merged in (step, env id) order and cut to the capacity -- the
    # rows the unsharded pool keeps --, moments added in shard order.
    def rollout_obs_keys(self) -> list[int]:
        return self.pools[0].rollout_obs_keys()

    def rollout_row_bytes(self) -> tuple[int, int]:
        return self.pools[0].rollout_row_bytes()

    @property
    def num_envs(self) -> int:
        return self.per * len(self.pools)

    def rollout_begin(self, horizon: int, episodes: int = 0, moments: bool = False) -> None:
        if self.pools[0].players != 1:
            raise RuntimeError("rollout not implemented for this environment")
        obs, act = self.rollout_row_bytes()
        native.check_rollout(horizon, episodes, moments, self.num_envs, obs, act)
        self._record_all(lambda p: p.rollout_begin(horizon, episodes, moments))
        self.rollout_horizon, self.rollout_capacity, self._rollout_cut = int(horizon), int(episodes), 0

    def rollout_shape(self) -> tuple[int, ...]:
        sh = list(self.pools[0].rollout_shape())
        sh[1] = self.num_envs
        return tuple(sh)

    def rollout_reset(self) -> list[np.ndarray]:
        return [np.concatenate(cols) for cols in zip(*self._record_all(lambda p: p.rollout_reset()))]

    def rollout_step(self, action: Any) -> list[np.ndarray]:
        action = np.asarray(action)
        if action.shape[:1] != (self.num_envs,):
            raise RuntimeError(f"Expected action of {self.num_envs} rows, got {action.shape}")
        rows: list[Any] = [None] * len(self.pools)

        def run(s: int, p: DevicePool, _: Any) -> None:
            rows[s] = p.rollout_step(action[s * self.per:(s + 1) * self.per])

        self._each(run, [slice(0, self.per)] * len(self.pools))
        return [np.concatenate(cols) for cols in zip(*rows)]

    def rollout_batch(self) -> dict[str, np.ndarray]:
        parts = self._record_all(lambda p: p.rollout_batch())
        return {name: np.concatenate([b[name] for b in parts], axis=1) for name in parts[0]}

    def rollout_gae(self, values: Any, gamma: float, lam: float) -> tuple[np.ndarray, np.ndarray]:
        native.check_rollout(self.rollout_horizon, 0, False, self.num_envs, values=values, gamma=gamma, lam=lam)
        out: list[Any] = [None] * len(self.pools)

        def run(s: int, p: DevicePool, _: Any) -> None:
            out[s] = p.rollout_gae(np.ascontiguousarray(values[:, s * self.per:(s + 1) * self.per]), gamma, lam)

        self._each(run, [slice(0, self.per)] * len(self.pools))
        return np.concatenate([o[0] for o in out], axis=1), np.concatenate([o[1] for o in out], axis=1)

    def rollout_counters(self) -> np.ndarray:
        c = np.array(self._record_all(lambda p: p.rollout_counters()))
        out = c[0].copy()
        out[0] = min(int(c[:, 0].sum()), self.rollout_capacity)
        out[1] = c[:, 1].sum()
        out[2] = c[:, 2].sum() + self._rollout_cut + int(c[:, 0].sum()) - out[0]
        return out

    def rollout_episodes(self) -> tuple[np.ndarray, ...]:
        cols = [np.concatenate(c) for c in zip(*self._record_all(lambda p: p.rollout_episodes()))]
        order = np.lexsort((cols[0], cols[1]))[:self.rollout_capacity]
        self._rollout_cut += len(cols[0]) - len(order)
        return tuple(c[order] for c in cols)

    def rollout_moments(self) -> np.ndarray:
        parts = self._record_all(lambda p: p.rollout_moments())
        out = parts[0].copy()
        for m in parts[1:]:
            out = out + m
        return out

    def rollout_next(self) -> None:
        self._record_all(lambda p: p.rollout_next())

    def rollout_end(self) -> None:
        self._record_all(lambda p: p.rollout_end())

    # -- rollout actor: one actor per shard.  The noise is keyed by the GLOBAL env id and the collector's step counter,
    # which every shard counts alike, so the shards' rows are the unsharded pool's --
    def actor_begin(self, actor: Any, seed: int = 0, deterministic: bool = False, actions: Any = None) -> None:
        self._record_all(lambda p: p.actor_begin(actor, seed, deterministic, actions))

    def actor_shape(self) -> tuple[int, ...]:
        return self.pools[0].actor_shape()

    def actor_end(self) -> None:
        self._record_all(lambda p: p.actor_end())

    def rollout_collect(self, steps: int = 0, wait: bool = True) -> None:
        self._record_all(lambda p: p.rollout_collect(steps, wait))

    def actor_batch(self) -> tuple[np.ndarray, np.ndarray]:
        parts = self._record_all(lambda p: p.actor_batch())
        return np.concatenate([a for a, _ in parts], axis=1), np.concatenate([b for _, b in parts], axis=1)

    def rollout_gae_stored(self, gamma: float, lam: float) -> tuple[np.ndarray, np.ndarray]:
        parts = self._record_all(lambda p: p.rollout_gae_stored(gamma, lam))
        return np.concatenate([a for a, _ in parts], axis=1), np.concatenate([b for _, b in parts], axis=1)

    def actor_eval(self, obs: Any, env_ids: Any, step: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Every row by the shard that holds its env."""
        obs = [obs] if isinstance(obs, np.ndarray) else [np.asarray(o) for o in obs]
        ids = np.ascontiguousarray(env_ids, np.int32).reshape(-1)
        shard = (ids - self.offset) // self.per
        bad = ids[(shard < 0) | (shard >= len(self.pools))]
        if len(bad):
            raise ValueError(f"env_id {int(bad[0])} out of range")
        p0 = self.pools[0]
        action = np.empty((len(ids), *p0.action_shape), dtype=p0.action_dtype)
        logp, value = np.empty(len(ids), np.float32), np.empty(len(ids), np.float32)
        for s, p in enumerate(self.pools):
            idx = np.flatnonzero(shard == s)
            if len(idx):
                action[idx], logp[idx], value[idx] = p.actor_eval([o[idx] for o in obs], ids[idx], step)
        return action, logp, value

    # -- self-play driver: one driver per shard; the keys take global env ids, so the shards play the unsharded pool's
    # games --
    def selfplay_begin(self, net: Any, **options: Any) -> None:
        native.check_selfplay(**options)
        for device in sorted({p.device for p in self.pools}):
            net._handle(device)  # one copy per device, made before the shards ask for it at once
        self._record_all(lambda p: p.selfplay_begin(net, **options))

    def selfplay_run(self, plies: int, wait: bool = True) -> None:
        """`DevicePool.selfplay_run` in every shard, each with the net's copy on its own device; shards on different
        devices run at once.  Shards that share a device share the net's copy and its policy and value rows, and calls
        that use one copy must not overlap ON THE DEVICE: such a shard takes its turn and is waited for before the turn
        passes, also with `wait=False` -- only a shard alone on its device is enqueue-only."""
        plies = native.check_selfplay_plies(plies)
        turn = {p.device: threading.Lock() for p in self.pools}
        shared = {d: sum(p.device == d for p in self.pools) > 1 for d in turn}

        def run(p: DevicePool) -> None:
            with turn[p.device]:
                p.selfplay_run(plies, wait or shared[p.device])

        self._guided = None
        self._record_all(run)

    def selfplay_stats(self) -> np.ndarray:
        """The shards' statistics added up; t is every shard's."""
        parts = self._record_all(lambda p: p.selfplay_stats())
        out = np.sum(parts, axis=0)
        out[5] = parts[0][5]
        return out

    def selfplay_end(self) -> None:
        self._record_all(lambda p: p.selfplay_end())

    def selfplay_noise(self) -> np.ndarray:
        """The shards' noise rows in env order."""
        return np.concatenate(self._record_all(lambda p: p.selfplay_noise()), axis=0)

    # -- arena: one per shard; the sides take GLOBAL env ids (every shard knows its offset), so the shards play the
    # unsharded pool's match.  selfplay_run and selfplay_end above drive and close it --
    def arena_begin(self, net_a: Any, net_b: Any, **options: Any) -> None:
        native.check_arena(net_a, net_b, **options)
        for device in sorted({p.device for p in self.pools}):
            net_a._handle(device)  # one copy of each net per device, made before the shards ask for them at once
            net_b._handle(device)
        self._record_all(lambda p: p.arena_begin(net_a, net_b, **options))

    def arena_run(self, plies: int, wait: bool = True) -> None:
        self.selfplay_run(plies, wait)

    def arena_stats(self) -> np.ndarray:
        """The shards' statistics added up; t is every shard's."""
        parts = self._record_all(lambda p: p.arena_stats())
        out = np.sum(parts, axis=0)
        out[7] = parts[0][7]
        return out

    def arena_end(self) -> None:
        self.selfplay_end()

    def net_eval_pair(self, net_a: Any, net_b: Any, obs: Any, mask: Any, status: Any, side: Any,
                      priors: bool = False) -> tuple:
        """`DevicePool.net_eval_pair` on the first shard: the rows are positions, whichever shard holds their envs."""
        return self.pools[0].net_eval_pair(net_a, net_b, obs, mask, status, side, priors)

    def close(self) -> None:
        self._exec.shutdown(wait=True)
        for p in self.pools:
            p.close()


def make_native_classes(fd: FamilyDef, static_action_spec: list | None = None) -> tuple[type, type]:
    """Build `_<Name>EnvSpec` and `_<Name>EnvPool` for a family.  `static_action_spec`: key
    list to use for the class-level `_action_keys` when `fd.action_spec` cannot be evaluated
    on the default config (Atari sizes its action set from the ROM)."""
    config_items = COMMON_CONFIG + list(fd.default_config) + EXTENSION_CONFIG
    config_keys = [k for k, _ in config_items]
    default_values = tuple(v for _, v in config_items)
    # key lists are static per class in the reference (py_envpool.h:163-171)
    default_conf = dict(config_items)
    state_keys = [k for k, _ in COMMON_STATE_SPEC] + [k for k, _ in fd.state_spec(default_conf)]
    action_keys = [k for k, _ in COMMON_ACTION_SPEC] + [
        k for k, _ in (static_action_spec or fd.action_spec(default_conf))]

    class _Spec:
        _config_keys = config_keys
        _default_config_values = default_values
        _state_keys = state_keys
        _action_keys = action_keys

        def __init__(self, config_values: Any) -> None:
            values = list(config_values)
            if len(values) != len(config_keys):
                raise TypeError(
                    f"{type(self).__name__} expects {len(config_keys)} config values"
                )
            conf = dict(zip(config_keys, values))
            # EnvSpec ctor, envpool/core/env_spec.h:75-83
            if conf["batch_size"] > conf["num_envs"]:
                raise ValueError(
                    "It is required that batch_size <= num_envs, got num_envs = "
                    f"{conf['num_envs']}, batch_size = {conf['batch_size']}"
                )
            if conf["batch_size"] == 0:
                conf["batch_size"] = conf["num_envs"]
            for key, supported in fd.unsupported.items():
                if conf.get(key, supported) != supported:
                    raise ValueError(
                        f"{fd.name}: {key}={conf[key]!r} is not supported by the "
                        f"MI355X engine yet (only {supported!r})"
                    )
            self._conf = conf
            self._config_values = tuple(conf[k] for k in config_keys)
            # like EnvSpec's ctor (env_spec.h:70-74) the specs are built -- and
            # their arguments validated -- at construction time
            fd.state_spec(conf)
            fd.action_spec(conf)
            fd.native_params(conf)

        @property
        def _state_spec(self) -> tuple:
            return tuple(s for _, s in COMMON_STATE_SPEC) + tuple(
                s for _, s in fd.state_spec(self._conf))

        @property
        def _action_spec(self) -> tuple:
            return tuple(s for _, s in COMMON_ACTION_SPEC) + tuple(
                s for _, s in fd.action_spec(self._conf))

    class _Pool:
        _state_keys = state_keys
        _action_keys = action_keys

        def __init__(self, spec: Any) -> None:
            conf = dict(zip(spec._config_keys, spec._config_values))
            if fd.players == 1:
                if conf["max_num_players"] != 1:
                    raise ValueError("only single-player envs are on the MI355X path")
            elif conf["max_num_players"] != fd.players:
                raise ValueError(f"{fd.name}: max_num_players must be {fd.players}, got {conf['max_num_players']}")
            params = {k: float(v) for k, v in fd.native_params(conf).items()}
            if conf["recv_timeout_ms"] != -1:
                params["recv_timeout_ms"] = float(conf["recv_timeout_ms"])
            kw = dict(
                batch_size=conf["batch_size"],
                seed=conf["seed"],
                env_seed=list(conf["env_seed"]) or None,
                max_episode_steps=conf["max_episode_steps"],
                env_id_offset=conf["env_id_offset"],
                params=params,
            )
            device = conf["device"]
            if fd.pool_factory is not None:
                if isinstance(device, (list, tuple)):
                    if len(device) != 1:
                        raise ValueError(f"{fd.name}: in-process sharding over several devices "
                                         "is not available for this family")
                    device = device[0]
                self._pool = fd.pool_factory(conf, dict(kw, device=int(device)))
            elif isinstance(device, (list, tuple)) and len(device) > 1:
                self._pool: Any = _ShardedPools(fd.native, list(device), conf["num_envs"], **kw)
            else:
                if isinstance(device, (list, tuple)):
                    device = device[0]
                self._pool = DevicePool(fd.native, conf["num_envs"], device=int(device), **kw)
            self._spec = spec
            # the C ABI's view of the layout must agree with the Python spec
            native_keys = [k for k, _, _ in self._pool.state_keys]
            assert native_keys == state_keys, (native_keys, state_keys)

        def _send(self, action: list[np.ndarray]) -> None:
            # list order = _action_keys: env_id, players.env_id, <env action>
            if fd.players > 1 and not np.array_equal(np.asarray(action[1]), np.asarray(action[0])):
                # divergence: the reference routes player action rows by players.env_id; here every env takes
                # the one action row of its env_id
                raise ValueError(f"{fd.name}: players.env_id must equal env_id (one action row per env)")
            self._pool.send(action[0], action[-1])

        def _recv(self) -> list[np.ndarray]:
            return self._pool.recv()

        def _reset(self, env_ids: np.ndarray) -> None:
            self._pool.reset(np.asarray(env_ids, dtype=np.int32))

        def _render(self, env_ids: np.ndarray, width: int, height: int,
                    camera_id: int) -> np.ndarray:
            # async_envpool.h:183-222; a family without a render kernel raises the reference's
            # RuntimeError("render not implemented for this environment") from the engine
            render = getattr(self._pool, "render", None)
            if render is None:  # a pool with its own executor
                raise RuntimeError("render not implemented for this environment")
            return render(env_ids, width, height, camera_id)

        def _snapshot(self, env_ids: Any, rng: bool) -> Any:
            return self._pool.snapshot(env_ids, rng)

        def _restore(self, blob: Any, env_ids: Any) -> None:
            self._pool.restore(blob, env_ids)

        def _fork(self, src: Any, dst: Any, rng: bool) -> None:
            self._pool.fork(src, dst, rng)

        def _playout(self, env_ids: Any, repeats: int, max_plies: int, seed: int, commit: bool) -> Any:
            playout = getattr(self._pool, "playout", None)
            if playout is None:  # a pool with its own executor
                raise RuntimeError("playout not implemented for this environment")
            return playout(env_ids, repeats, max_plies, seed, commit)

        def _search(self, env_ids: Any, simulations: int, leaf_playouts: int, c_puct: float, max_plies: int,
                    seed: int) -> Any:
            search = getattr(self._pool, "search", None)
            if search is None:  # a pool with its own executor
                raise RuntimeError("search not implemented for this environment")
            return search(env_ids, simulations, leaf_playouts, c_puct, max_plies, seed)

        def _solve(self, env_ids: Any, depth: int, max_nodes: int, table_bits: int = 0) -> Any:
            solve = getattr(self._pool, "solve", None)
            if solve is None:  # a pool with its own executor
                raise RuntimeError("solve not implemented for this environment")
            if table_bits == 0:  # today's call
                return solve(env_ids, depth, max_nodes)
            return solve(env_ids, depth, max_nodes, table_bits)

        def _guided(self) -> Any:
            if getattr(self._pool, "guided_begin", None) is None:  # a pool with its own executor
                raise RuntimeError("guided search not implemented for this environment")
            return self._pool

        def _gumbel(self) -> Any:
            if getattr(self._pool, "gumbel_begin", None) is None:  # a pool with its own executor
                raise RuntimeError("gumbel search not implemented for this environment")
            return self._pool

        def _recorder(self) -> Any:
            if getattr(self._pool, "record_begin", None) is None:  # a pool with its own executor
                raise RuntimeError("recorder not implemented for this environment")
            return self._pool

        def _rollout(self) -> Any:
            # a pool with its own executor (Atari), or one with a row per player (the PGX games)
            if getattr(self._pool, "rollout_begin", None) is None or fd.players != 1:
                raise RuntimeError("rollout not implemented for this environment")
            return self._pool

        def _selfplay(self) -> Any:
            if getattr(self._pool, "selfplay_begin", None) is None:  # a pool with its own executor
                raise RuntimeError("guided search not implemented for this environment")
            return self._pool

        def _xla(self) -> Any:
            raise RuntimeError("XLA is not available for the MI355X engine")

        def close(self) -> None:
            self._pool.close()

        @property
        def device_pool(self) -> Any:
            """Extension: the underlying DevicePool (zero-copy device path)."""
            return self._pool

    _Spec.__name__ = _Spec.__qualname__ = f"_{fd.name}EnvSpec"
    _Pool.__name__ = _Pool.__qualname__ = f"_{fd.name}EnvPool"
    return _Spec, _Pool
