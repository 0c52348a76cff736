"""Zero-copy views of a pool's device-resident result batch as torch tensors
(the analogue of the reference's XLA path, envpool/core/xla.h, without its
host staging).  torch is only imported here.

Errors a step kernel reports through its pool's error word (MiniGrid: a reset's rejection sampling ran out of
`minigrid_max_tries`) reach this path late: `recv_device` does not wait for the kernel it hands out, so it
raises only for kernels already finished -- one recv later, or at `pool.synchronize()`.  The host path (`recv`)
waits and raises for the batch itself.  The word is sticky: every later recv of that pool raises too, and the
pool has to be recreated."""

from __future__ import annotations

import collections
from typing import Any

import numpy as np

from envpool_amd.core import native

_TYPESTR = {np.dtype(np.int32): "<i4", np.dtype(np.float32): "<f4",
            np.dtype(np.float64): "<f8", np.dtype(np.bool_): "|b1",
            np.dtype(np.uint8): "|u1", np.dtype(np.int8): "|i1", np.dtype(np.int64): "<i8"}


class _DevArray:
    def __init__(self, ptr: int, shape: tuple, dtype: Any) -> None:
        self.__cuda_array_interface__ = {
            "shape": tuple(int(s) for s in shape),
            "typestr": _TYPESTR[np.dtype(dtype)],
            "data": (int(ptr), False),
            "version": 2,
        }


def send_device_tensors(pool: Any, action: Any, env_id: Any = None) -> None:
    """Step the envs with an action tensor that lives on the pool's device.  The step
    kernel is ordered behind everything enqueued so far on torch's CURRENT stream
    (the stream the learner produced `action` on) -- no host synchronisation.
    `action=None` resets the listed envs."""
    import torch

    k = None
    d_action = None
    if action is not None:
        if not action.is_contiguous() or action.dtype != _torch_dtype(pool.action_dtype):
            raise RuntimeError(
                f"send_device_tensors: action must be contiguous {np.dtype(pool.action_dtype)}")
        d_action = action.data_ptr()
        k = int(action.shape[0])
    d_ids = None
    if env_id is not None:
        if env_id.dtype != torch.int32 or not env_id.is_contiguous():
            raise RuntimeError("send_device_tensors: env_id must be contiguous int32")
        d_ids = env_id.data_ptr()
        k = int(env_id.shape[0])
    dev = torch.device("cuda", pool.device)
    pool.wait_stream(torch.cuda.current_stream(dev).cuda_stream)
    pool.send_device(d_action, k, d_ids)
    # The step kernel reads both tensors on the pool's PRIVATE stream, which torch's caching
    # allocator knows nothing about: a temporary the caller drops right after this call
    # (`send_device_tensors(pool, policy(obs))`) could be handed to a later kernel on torch's stream
    # while the step kernel is still reading it.  So the pool keeps a reference to what it was
    # sent until an event recorded behind the step kernel has passed.  (Not `Tensor.record_stream`:
    # that makes the allocator record an event on the pool's stream when the tensor is freed --
    # possibly after the pool, and its stream, are gone.)
    sent = pool.__dict__.setdefault("_sent_tensors", collections.deque())
    while sent and sent[0][0].query():
        sent.popleft()
    if action is not None or env_id is not None:
        ev = torch.cuda.Event()
        ev.record(torch.cuda.ExternalStream(pool.stream, device=dev))
        sent.append((ev, action, env_id))


def _torch_dtype(dt: Any) -> Any:
    import torch

    return {np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32,
            np.dtype(np.float64): torch.float64}[np.dtype(dt)]


def recv_device_tensors(pool: Any, device: Any = None, order_current_stream: bool = True
                        ) -> dict[str, Any]:
    """pool.recv_device() -> {state key: torch tensor aliasing the batch}.
    Valid until the second next recv_device on the pool.  With
    `order_current_stream` torch's current stream is made to wait for the step
    kernel, so the tensors can be consumed right away without a host sync."""
    import torch

    ptrs, k = pool.recv_device()
    dev = torch.device("cuda", pool.device) if device is None else device
    if order_current_stream:
        pool.consumer_wait(torch.cuda.current_stream(dev).cuda_stream)
    out = {}
    for i, ((name, dtype, _), ptr) in enumerate(zip(pool.state_keys, ptrs)):
        if k == 0:
            continue
        # a per-player key of a multi-player family: its [k, P, ...] block as [k * P, ...] player rows
        out[name] = torch.as_tensor(_DevArray(ptr, pool.view_shape(i, k), dtype), device=dev)
    return out


def render_device(pool: Any, env_ids: Any, width: int = 0, height: int = 0, camera_id: int = -1,
                  out: Any = None) -> Any:
    """`pool.render` without the way down: a torch.uint8 [k, H, W, 3] tensor on the pool's device, painted by the
    render kernel straight into torch's memory (no PCIe transfer, no host synchronisation).  The kernel is ordered
    behind torch's CURRENT stream (whatever still uses the memory there) and the current stream behind the kernel,
    so the tensor can be consumed right away.  `out`: a contiguous uint8 tensor of that many bytes to paint into
    (any storage offset) instead of a fresh one."""
    import torch

    ids = np.ascontiguousarray(env_ids, dtype=np.int32).reshape(-1)
    w, h = pool.render_size(width, height)
    dev = torch.device("cuda", pool.device)
    shape = (len(ids), h, w, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() != int(np.prod(shape)) \
            or out.device != dev:
        raise RuntimeError(f"render_device: out must be a contiguous uint8 tensor of {shape} on {dev}")
    cur = torch.cuda.current_stream(dev)
    pool.wait_stream(cur.cuda_stream)
    pool.render_device(out.data_ptr(), ids, width, height, camera_id)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.ExternalStream(pool.stream, device=dev))
    cur.wait_event(ev)
    return out.view(shape)


def _order_both_ways(pool: Any, dev: Any, launch: Any) -> None:
    """The pool's stream behind torch's CURRENT stream, `launch()`, the current stream behind the pool's stream."""
    import torch

    cur = torch.cuda.current_stream(dev)
    pool.wait_stream(cur.cuda_stream)
    launch()
    ev = torch.cuda.Event()
    ev.record(torch.cuda.ExternalStream(pool.stream, device=dev))
    cur.wait_event(ev)


def snapshot_device(pool: Any, env_ids: Any = None, rng: bool = True, out: Any = None) -> Any:
    """`pool.snapshot` without the way down: the blob as a torch.uint8 tensor on the pool's device, written by the
    snapshot kernels straight into torch's memory (no PCIe transfer, no host synchronisation), ordered against torch's
    current stream like `render_device`.  `out`: a contiguous, 16-byte aligned uint8 tensor of at least
    `pool.snapshot_bytes(k, rng)` bytes to write into.  The tensor remembers its header (`restore_device` needs it on
    the host); a copy of the tensor does not, and costs `restore_device` a 64-byte read from the device."""
    import torch

    k = pool.num_envs if env_ids is None else len(np.asarray(env_ids).reshape(-1))
    nbytes = pool.snapshot_bytes(k, rng)
    dev = torch.device("cuda", pool.device)
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() < nbytes or out.device != dev \
            or out.data_ptr() % 16 != 0:
        raise RuntimeError(f"snapshot_device: out must be a contiguous, 16-byte aligned uint8 tensor of at least "
                           f"{nbytes} bytes on {dev}")
    blob = out.view(-1)[:nbytes]
    header: list = []
    _order_both_ways(pool, dev, lambda: header.append(pool.snapshot_device(blob.data_ptr(), env_ids, rng)))
    blob._epa_snapshot_header = header[0]
    return blob


def restore_device(pool: Any, blob: Any, env_ids: Any = None) -> None:
    """`pool.restore` from a blob that lives on the pool's device (`snapshot_device` of this or another pool of the
    same family), stream-ordered like `snapshot_device`.  `env_ids=None`: envs 0 .. k-1, k from the blob."""
    import torch

    dev = torch.device("cuda", pool.device)
    if blob.dtype != torch.uint8 or not blob.is_contiguous() or blob.device != dev or blob.dim() != 1:
        raise RuntimeError(f"restore_device: blob must be a contiguous one-dimensional uint8 tensor on {dev}")
    header = getattr(blob, "_epa_snapshot_header", None)
    if header is None:
        if blob.numel() < 64:
            raise ValueError(f"snapshot blob of {blob.numel()} bytes is shorter than a header")
        header = blob[:64].cpu().numpy().tobytes()
    total = int(np.frombuffer(header, dtype="<u8", count=1, offset=48)[0])
    if blob.numel() < total:
        raise ValueError(f"snapshot blob of {blob.numel()} bytes is shorter than its header says ({total})")
    _order_both_ways(pool, dev, lambda: pool.restore_device(blob.data_ptr(), header, env_ids))


def fork(pool: Any, src: Any, dst: Any, rng: bool = True) -> None:
    """`pool.fork` ordered against torch's current stream: behind what torch has enqueued, and in front of what it
    enqueues next."""
    import torch

    _order_both_ways(pool, torch.device("cuda", pool.device), lambda: pool.fork(src, dst, rng))


def playout_device(pool: Any, env_ids: Any = None, repeats: int = 1, max_plies: int = 0, seed: int = 0,
                   commit: bool = False) -> tuple[Any, Any, Any]:
    """`pool.playout` without the way down: (returns float32 [k, R, 2], plies int32 [k, R], status uint8 [k, R]) as
    torch tensors on the pool's device, written by the playout kernel straight into torch's memory (no PCIe transfer,
    no host synchronisation) and ordered against torch's current stream like `snapshot_device`: the kernel behind what
    torch has enqueued, the current stream behind the kernel.  With `commit` a step sent afterwards sees the final
    positions."""
    import torch

    if env_ids is None:
        env_ids = np.arange(pool.env_id_offset, pool.env_id_offset + pool.num_envs, dtype=np.int32)
    ids = native.check_playout(env_ids, repeats, max_plies, commit)
    k, r = len(ids), int(repeats)
    dev = torch.device("cuda", pool.device)
    returns = torch.empty((k, r, 2), dtype=torch.float32, device=dev)
    plies = torch.empty((k, r), dtype=torch.int32, device=dev)
    status = torch.empty((k, r), dtype=torch.uint8, device=dev)
    _order_both_ways(pool, dev, lambda: pool.playout_device(returns.data_ptr(), plies.data_ptr(), status.data_ptr(),
                                                            ids, repeats, max_plies, seed, commit))
    return returns, plies, status


def search_device(pool: Any, env_ids: Any = None, simulations: int = 64, leaf_playouts: int = 8, c_puct: float = 1.25,
                  max_plies: int = 0, seed: int = 0) -> tuple[Any, Any, Any]:
    """`pool.search` without the way down: (visits int32 [k, A], returns int32 [k, A], action int32 [k]) as torch
    tensors on the pool's device, written by the search kernel straight into torch's memory (no PCIe transfer, no host
    synchronisation) and ordered against torch's current stream like `playout_device`."""
    import torch

    if env_ids is None:
        env_ids = np.arange(pool.env_id_offset, pool.env_id_offset + pool.num_envs, dtype=np.int32)
    ids = native.check_search(env_ids, simulations, leaf_playouts, c_puct, max_plies)
    k, a = len(ids), pool.search_actions()
    dev = torch.device("cuda", pool.device)
    visits = torch.empty((k, a), dtype=torch.int32, device=dev)
    returns = torch.empty((k, a), dtype=torch.int32, device=dev)
    action = torch.empty((k,), dtype=torch.int32, device=dev)
    _order_both_ways(pool, dev, lambda: pool.search_device(visits.data_ptr(), returns.data_ptr(), action.data_ptr(),
                                                           ids, simulations, leaf_playouts, c_puct, max_plies, seed))
    return visits, returns, action


def solve_device(pool: Any, env_ids: Any = None, depth: int = 0, max_nodes: int = 1 << 20,
                 table_bits: int = 0) -> tuple[Any, Any, Any, Any, Any]:
    """`pool.solve` without the way down: (value int8 [k], q int8 [k, A], action int32 [k], status uint8 [k], nodes
    int64 [k]) as torch tensors on the pool's device, written by the solve kernel straight into torch's memory (no PCIe
    transfer, no host synchronisation: the call only enqueues) and ordered against torch's current stream like
    `search_device`.  `table_bits`: the lanes' transposition tables (`DevicePool.solve`); 0: none."""
    import torch

    if env_ids is None:
        env_ids = np.arange(pool.env_id_offset, pool.env_id_offset + pool.num_envs, dtype=np.int32)
    ids = native.check_solve(env_ids, depth, max_nodes, table_bits)
    k, a = len(ids), pool.solve_actions()
    dev = torch.device("cuda", pool.device)
    value = torch.empty((k,), dtype=torch.int8, device=dev)
    q = torch.empty((k, a), dtype=torch.int8, device=dev)
    action = torch.empty((k,), dtype=torch.int32, device=dev)
    status = torch.empty((k,), dtype=torch.uint8, device=dev)
    nodes = torch.empty((k,), dtype=torch.int64, device=dev)
    _order_both_ways(pool, dev, lambda: pool.solve_device(value.data_ptr(), q.data_ptr(), action.data_ptr(),
                                                          status.data_ptr(), nodes.data_ptr(), ids, depth, max_nodes,
                                                          table_bits))
    return value, q, action, status, nodes


def _guided_round_device(pool: Any, evaluate: Any, dev: Any, k: int, simulations: int, leaves: tuple,
                         what: str, width: int = 0, advances: Any = None) -> tuple[Any, Any, Any]:
    """simulations + 1 advances from the emitted `leaves` and the result, every launch ordered both ways.  A wide
    session (`width` slots per root; the leaves have k * width rows): `advances` launches without a host wait, or
    (None) as many as the round needs, found by reading one reduced status byte per launch."""
    import torch

    obs, mask, status = leaves
    a = mask.shape[1]
    rows = k * width if width else k
    most = int(simulations) + 1
    if width and advances is not None:
        if isinstance(advances, bool) or int(advances) != advances or not 1 <= int(advances) <= most:
            pool.guided_end()
            raise ValueError(f"{what}: advances = {advances} must be 1 .. simulations + 1 = {most}")
        most = int(advances)
    if getattr(evaluate, "_is_epa_net", False):  # the built-in network: the whole round is enqueued from C++
        _order_both_ways(pool, dev, lambda: pool.net_run_device(evaluate, obs.data_ptr(), mask.data_ptr(),
                                                                status.data_ptr(), advances))
        most = 0
    for _ in range(most):
        if width and advances is None and not bool((status != 2).any().item()):
            break  # the round is complete: nothing is pending
        priors, values = evaluate(obs, mask, status)
        priors = priors.to(device=dev, dtype=torch.float32).contiguous()
        values = values.to(device=dev, dtype=torch.float32).contiguous().view(-1)
        if tuple(priors.shape) != (rows, a) or tuple(values.shape) != (rows,):
            pool.guided_end()
            raise ValueError(f"{what}: evaluate returned priors {tuple(priors.shape)} and values "
                             f"{tuple(values.shape)} for a session of [{rows}, {a}]")
        _order_both_ways(pool, dev, lambda: pool.guided_advance_device(priors.data_ptr(), values.data_ptr(), rows,
                                                                       obs.data_ptr(), mask.data_ptr(),
                                                                       status.data_ptr()))
    visits = torch.empty((k, a), dtype=torch.int32, device=dev)
    vals = torch.empty((k, a), dtype=torch.float32, device=dev)
    action = torch.empty((k,), dtype=torch.int32, device=dev)
    _order_both_ways(pool, dev, lambda: pool.guided_result_device(visits.data_ptr(), vals.data_ptr(),
                                                                  action.data_ptr()))
    return visits, vals, action


def guided_search_device(pool: Any, evaluate: Any, env_ids: Any = None, simulations: int = 64,
                         c_puct: float = 1.25, nodes: Any = None, keep_open: bool = False, width: Any = None,
                         advances: Any = None, tactics: int = 0,
                         tactics_nodes: int = native.GUIDED_TACTICS_NODES, prove: bool = False) -> tuple[Any, Any, Any]:
    """A whole guided search (`pool.guided_begin` ..) with the evaluator on the device: `evaluate(obs, mask, status)`
    gets torch tensors on the pool's device (bool [k, H, W, C], bool [k, A], uint8 [k]) written by the search kernels
    and returns (priors float32 [k, A], values float32 [k]) there; nothing crosses PCIe and the host never waits.
    Every launch is ordered against torch's current stream like `search_device`: the kernel behind what torch has
    enqueued (the evaluator), the current stream behind the kernel.  Returns (visits int32 [k, A], values float32
    [k, A], action int32 [k]) on the device and closes the session -- or, with `keep_open`, leaves it open for
    `guided_reroot_device`; `nodes` is the node capacity per root (`DevicePool.guided_begin`).
    `width` = W (1 .. 32) opens a wide session: `evaluate` gets and returns k W rows, flattened (row i W + j is slot j
    of root i; a slot of status 2 has nothing pending), so a model function written for the plain session works
    unchanged.  `advances=None` reads one reduced status byte per launch -- the one host wait -- and stops when the
    round is complete; an integer makes exactly that many advances with no host wait: roots that are not finished then
    simply have fewer visits, which the result shows.
    `tactics` = D (1 .. 16), `tactics_nodes`: the exact leaf status (`DevicePool.guided_begin`): the solver's launch
    is enqueued behind every advance, so `evaluate` sees decided leaves as rows of status 1; the session keeps it
    through `guided_reroot_device`, and `guided_decided_device` gives the counters (before the session is closed).
    `prove` = True: proven values (`DevicePool.guided_begin`); a proven root's rows have status 2 for the rest of the
    round, the session keeps the flag through `guided_reroot_device`, and `guided_proof_device` reads the proofs
    (before the session is closed)."""
    import torch

    if env_ids is None:
        env_ids = np.arange(pool.env_id_offset, pool.env_id_offset + pool.num_envs, dtype=np.int32)
    ids = native.check_guided(env_ids, simulations, c_puct)
    native.check_guided_nodes(simulations, nodes)
    width = native.check_guided_width(width)
    tactics, tactics_nodes = native.check_guided_tactics(tactics, tactics_nodes)
    prove = native.check_guided_prove(prove)
    if advances is not None and not width:
        raise ValueError("guided_search_device: advances is an argument of a wide session (width=)")
    h, w, c, a = pool.guided_shape()
    k = len(ids)
    rows = k * width if width else k
    dev = torch.device("cuda", pool.device)
    obs = torch.empty((rows, h, w, c), dtype=torch.bool, device=dev)
    mask = torch.empty((rows, a), dtype=torch.bool, device=dev)
    status = torch.empty((rows,), dtype=torch.uint8, device=dev)
    _order_both_ways(pool, dev, lambda: pool.guided_begin_device(obs.data_ptr(), mask.data_ptr(), status.data_ptr(),
                                                                 ids, simulations, c_puct, int(nodes or 0),
                                                                 width or None, tactics, tactics_nodes, prove))
    out = _guided_round_device(pool, evaluate, dev, k, simulations, (obs, mask, status), "guided_search_device",
                               width, advances)
    if not keep_open:
        pool.guided_end()
    return out


def guided_decided_device(pool: Any) -> Any:
    """int32 [k] on the pool's device: the leaves the exact leaf status (`tactics=`) decided per root of the pool's
    open PUCT session since it began; a reroot does not reduce it.  Only enqueued, ordered both ways against torch's
    current stream."""
    import torch

    k = pool._guided_open("guided_decided", "puct")
    dev = torch.device("cuda", pool.device)
    decided = torch.empty((k,), dtype=torch.int32, device=dev)
    _order_both_ways(pool, dev, lambda: pool.guided_decided_device(decided.data_ptr()))
    return decided


def guided_proof_device(pool: Any) -> tuple[Any, Any]:
    """(value int8 [k], q int8 [k, A]) on the pool's device: the proven values (`prove=True`) of the roots of the
    pool's open PUCT session and of the children of their actions, -128 for none (`DevicePool.guided_proof`).  Only
    enqueued, ordered both ways against torch's current stream."""
    import torch

    k = pool._guided_open("guided_proof", "puct")
    dev = torch.device("cuda", pool.device)
    value = torch.empty((k,), dtype=torch.int8, device=dev)
    q = torch.empty((k, pool.guided_shape()[3]), dtype=torch.int8, device=dev)
    _order_both_ways(pool, dev, lambda: pool.guided_proof_device(value.data_ptr(), q.data_ptr()))
    return value, q


def guided_reroot_device(pool: Any, evaluate: Any, actions: Any, simulations: int,
                         advances: Any = None) -> tuple[Any, Any, Any]:
    """The next round of the pool's open PUCT session (`guided_search_device(..., keep_open=True)`) with tree reuse:
    `actions` is an int32 tensor [k] on the pool's device, the moves played -- `pool.guided_reroot_device` keeps their
    subtrees --, then `simulations` + 1 advances with `evaluate` and the result, every launch ordered both ways against
    torch's current stream as in `guided_search_device`.  Returns (visits, values, action) on the device and leaves the
    session open.  A wide session keeps its width; `advances` as in `guided_search_device`.  The reroot kernel cannot
    know whether slots are still pending: they are dropped and nothing of them is backed up, so finish the round first
    (`advances=None`, or enough of them)."""
    import torch

    dev = torch.device("cuda", pool.device)
    h, w, c, a = pool.guided_shape()
    if actions.dtype != torch.int32 or actions.device != dev or actions.dim() != 1 or not actions.is_contiguous():
        raise ValueError(f"guided_reroot_device: actions must be a contiguous one-dimensional int32 tensor on {dev}")
    k = int(actions.shape[0])
    width = int(getattr(pool, "_guided_width", 0) or 0)
    if advances is not None and not width:
        raise ValueError("guided_reroot_device: advances is an argument of a wide session (width=)")
    rows = k * width if width else k
    obs = torch.empty((rows, h, w, c), dtype=torch.bool, device=dev)
    mask = torch.empty((rows, a), dtype=torch.bool, device=dev)
    status = torch.empty((rows,), dtype=torch.uint8, device=dev)
    _order_both_ways(pool, dev, lambda: pool.guided_reroot_device(actions.data_ptr(), k, simulations, obs.data_ptr(),
                                                                  mask.data_ptr(), status.data_ptr()))
    return _guided_round_device(pool, evaluate, dev, k, simulations, (obs, mask, status), "guided_reroot_device",
                                width, advances)


def gumbel_search_device(pool: Any, evaluate: Any, env_ids: Any = None, simulations: int = 32, max_considered: int = 16,
                         gumbel: Any = None, seed: Any = None, c_visit: float = 50.0,
                         c_scale: float = 0.1, batch: Any = None,
                         advances: Any = None) -> tuple[Any, Any, Any, Any]:
    """A whole Gumbel search (`pool.gumbel_begin` ..) with the evaluator on the device, as `guided_search_device`:
    `evaluate(obs, mask, status)` gets torch tensors on the pool's device and returns (logits float32 [k, A], values
    float32 [k]) there; nothing crosses PCIe and the host never waits.  `gumbel` is a float32 [k, A] tensor on the
    pool's device, or None: torch draws Gumbel(0, 1) noise there (from a generator seeded with `seed`, or torch's
    default one).  Returns (visits int32 [k, A], values float32 [k, A], action int32 [k], weights float32 [k, A]) on
    the device and closes the session.
    `batch` = B (1 .. 32) opens a batch session, a halving level per launch: `evaluate` gets and returns k B rows,
    flattened (row i B + j is slot j of root i; a slot of status 2 has nothing pending), so a model function written
    for the plain session works unchanged.  `advances=None` reads one reduced status byte per launch -- the one host
    wait -- and stops when the round is complete; an integer makes exactly that many advances with no host wait: roots
    that are not finished then simply have fewer visits, which the result shows."""
    import torch

    if env_ids is None:
        env_ids = np.arange(pool.env_id_offset, pool.env_id_offset + pool.num_envs, dtype=np.int32)
    ids = native.check_gumbel(env_ids, simulations, max_considered, c_visit, c_scale)
    batch = native.check_gumbel_batch(batch)
    if advances is not None and not batch:
        raise ValueError("gumbel_search_device: advances is an argument of a batch session (batch=)")
    most = int(simulations) + 1
    if advances is not None:
        if isinstance(advances, bool) or int(advances) != advances or not 1 <= int(advances) <= most:
            raise ValueError(f"gumbel_search_device: advances = {advances} must be 1 .. simulations + 1 = {most}")
        most = int(advances)
    a = pool.gumbel_actions()
    h, w, c, _ = pool.guided_shape()
    k = len(ids)
    dev = torch.device("cuda", pool.device)
    if gumbel is None:
        gen = None if seed is None else torch.Generator(device=dev).manual_seed(int(seed))
        u = torch.rand((k, a), dtype=torch.float32, device=dev, generator=gen).clamp_(1e-20, 1.0 - 1e-7)
        gumbel = -torch.log(-torch.log(u))
    gumbel = gumbel.to(device=dev, dtype=torch.float32).contiguous()
    if tuple(gumbel.shape) != (k, a):
        raise ValueError(f"gumbel_begin: gumbel of shape {tuple(gumbel.shape)} for a session of [{k}, {a}]")
    rows = k * batch if batch else k
    obs = torch.empty((rows, h, w, c), dtype=torch.bool, device=dev)
    mask = torch.empty((rows, a), dtype=torch.bool, device=dev)
    status = torch.empty((rows,), dtype=torch.uint8, device=dev)
    _order_both_ways(pool, dev, lambda: pool.gumbel_begin_device(gumbel.data_ptr(), obs.data_ptr(), mask.data_ptr(),
                                                                 status.data_ptr(), ids, simulations, max_considered,
                                                                 c_visit, c_scale, batch or None))
    if getattr(evaluate, "_is_epa_net", False):  # the built-in network: the whole round is enqueued from C++
        _order_both_ways(pool, dev, lambda: pool.net_run_device(evaluate, obs.data_ptr(), mask.data_ptr(),
                                                                status.data_ptr(), advances))
        most = 0
    for _ in range(most):
        if batch and advances is None and not bool((status != 2).any().item()):
            break  # the round is complete: nothing is pending
        logits, values = evaluate(obs, mask, status)
        logits = logits.to(device=dev, dtype=torch.float32).contiguous()
        values = values.to(device=dev, dtype=torch.float32).contiguous().view(-1)
        if tuple(logits.shape) != (rows, a) or tuple(values.shape) != (rows,):
            pool.guided_end()
            raise ValueError(f"gumbel_search_device: evaluate returned logits {tuple(logits.shape)} and values "
                             f"{tuple(values.shape)} for a session of [{rows}, {a}]")
        _order_both_ways(pool, dev, lambda: pool.gumbel_advance_device(logits.data_ptr(), values.data_ptr(), rows,
                                                                       obs.data_ptr(), mask.data_ptr(),
                                                                       status.data_ptr()))
    visits = torch.empty((k, a), dtype=torch.int32, device=dev)
    vals = torch.empty((k, a), dtype=torch.float32, device=dev)
    action = torch.empty((k,), dtype=torch.int32, device=dev)
    weights = torch.empty((k, a), dtype=torch.float32, device=dev)
    _order_both_ways(pool, dev, lambda: pool.gumbel_result_device(visits.data_ptr(), vals.data_ptr(),
                                                                  action.data_ptr(), weights.data_ptr()))
    pool.guided_end()
    return visits, vals, action, weights


def _record_rows(what: str, t: Any, dtypes: tuple, shape: tuple, dev: Any) -> None:
    if t.dtype not in dtypes or not t.is_contiguous() or tuple(t.shape) != shape or t.device != dev:
        raise RuntimeError(f"{what} must be a contiguous {dtypes[0]} tensor of shape {shape} on {dev}")


def selfplay_device(pool: Any, net: Any, plies: int, **options: Any) -> None:
    """`plies` plies of the pool's self-play driver (`DevicePool.selfplay_run(plies, wait=False)`), only enqueued and
    ordered both ways with torch's current stream like the other device forms: what torch enqueued before (a `Net`'s
    weights do not change, but the recorder's view or the envs may have been touched) is seen by the plies, and torch
    work enqueued afterwards -- reading `recorder_view_device`'s tensors, say -- sees their samples.  With `options`
    (`native.check_selfplay`'s, `dirichlet_alpha`, `dirichlet_eps` and `temperature` of a PUCT driver included), or
    when the pool's driver was not opened with `net`, the driver is opened first; otherwise the open one continues.
    `pool.selfplay_stats()` waits and reads the statistics, `pool.selfplay_noise()` the last ply's noise rows."""
    import torch

    plies = native.check_selfplay_plies(plies)
    if options or getattr(pool, "_selfplay_net", None) is not net:
        pool.selfplay_begin(net, **options)
    dev = torch.device("cuda", pool.device)
    _order_both_ways(pool, dev, lambda: pool.selfplay_run(plies, wait=False))


def arena_device(pool: Any, net_a: Any, net_b: Any, plies: int, **options: Any) -> None:
    """`selfplay_device` for an arena (`DevicePool.arena_run(plies, wait=False)`): only enqueued and ordered both ways
    with torch's current stream.  With `options` (`native.check_arena`'s), or when the pool's driver was not opened as
    an arena of these two nets, the arena is opened first; otherwise the open one continues.  `pool.arena_stats()`
    waits and reads the statistics."""
    import torch

    plies = native.check_selfplay_plies(plies)
    held = getattr(pool, "_selfplay_net", None)
    if options or not (isinstance(held, tuple) and held[0] is net_a and held[1] is net_b):
        pool.arena_begin(net_a, net_b, **options)
    dev = torch.device("cuda", pool.device)
    _order_both_ways(pool, dev, lambda: pool.arena_run(plies, wait=False))


def recorder_add_device(pool: Any, policy: Any, env_ids: Any = None) -> None:
    """`pool.record_add` with the policy targets where the model left them: `policy` is a float32 [k, A] tensor on the
    pool's device, read by the recorder's kernel (no PCIe transfer, no host synchronisation) and ordered against
    torch's current stream like `playout_device`.  The ids (host, global; None: the whole pool) must not repeat."""
    import torch

    if env_ids is None:
        env_ids = np.arange(pool.env_id_offset, pool.env_id_offset + pool.num_envs, dtype=np.int32)
    ids = native.check_record_ids("recorder add", env_ids)
    dev = torch.device("cuda", pool.device)
    _record_rows("recorder_add_device: policy", policy, (torch.float32,), (len(ids), pool.record_shape()[3]), dev)
    _order_both_ways(pool, dev, lambda: pool.record_add_device(policy.data_ptr(), ids))


def recorder_finish_device(pool: Any, reward: Any, done: Any, env_ids: Any = None) -> None:
    """`pool.record_finish` with what the step returned on the device: `reward` float32 [k, 2] (or [2 k], the
    per-player rows of `recv_device_tensors`) and `done` bool or uint8 [k].  Only enqueued, and ordered both ways with
    torch's current stream.  The ids (host, global; None: the whole pool) must not repeat."""
    import torch

    if env_ids is None:
        env_ids = np.arange(pool.env_id_offset, pool.env_id_offset + pool.num_envs, dtype=np.int32)
    ids = native.check_record_ids("recorder finish", env_ids)
    dev = torch.device("cuda", pool.device)
    k = len(ids)
    _record_rows("recorder_finish_device: reward", reward, (torch.float32,), (2 * k,) if reward.dim() == 1 else (k, 2),
                 dev)
    _record_rows("recorder_finish_device: done", done, (torch.bool, torch.uint8), (k,), dev)
    _order_both_ways(pool, dev, lambda: pool.record_finish_device(reward.data_ptr(), done.data_ptr(), ids))


def recorder_view_device(pool: Any) -> tuple[tuple, Any]:
    """The recorder's sample buffer as torch tensors that alias it -- (obs bool [capacity, H, W, C], mask bool
    [capacity, A], policy float32 [capacity, A], value float32, ply int32, env_id int32, sym uint8 [capacity]) -- and
    the int32 [1] count tensor: rows at and above the count are undefined.  Torch's current stream is made to wait for
    the recorder's launches so far; the tensors stay valid until the recorder is closed or replaced, and what a later
    `recorder_finish_device` writes is ordered by that call."""
    import torch

    h, w, c, a, _ = pool.record_shape()
    ptrs, count = pool.record_view_device()
    n = pool.record_capacity
    dev = torch.device("cuda", pool.device)
    shapes = [((n, h, w, c), np.bool_), ((n, a), np.bool_), ((n, a), np.float32), ((n,), np.float32),
              ((n,), np.int32), ((n,), np.int32), ((n,), np.uint8)]
    _order_both_ways(pool, dev, lambda: None)
    arrays = tuple(torch.as_tensor(_DevArray(p, s, d), device=dev) for p, (s, d) in zip(ptrs, shapes))
    return arrays, torch.as_tensor(_DevArray(count, (1,), np.int32), device=dev)


def recorder_clear(pool: Any) -> None:
    """Sets the recorder's sample count to 0 -- the device form of `drain`, once the caller has consumed the view's
    rows on torch's current stream; ordered both ways with it."""
    import torch

    _order_both_ways(pool, torch.device("cuda", pool.device), pool.record_clear)


# -- rollout collector (csrc/rollout.hip.h): the device forms.  They only enqueue on the pool's stream and are ordered
# both ways with torch's current stream. --
def _rollout_tensors(pool: Any, ptrs: list, k: int, dev: Any) -> dict[str, Any]:
    import torch

    return {name: torch.as_tensor(_DevArray(ptr, pool.view_shape(i, k), dtype), device=dev)
            for i, ((name, dtype, _), ptr) in enumerate(zip(pool.state_keys, ptrs))}


def rollout_reset_device(pool: Any) -> dict[str, Any]:
    """`pool.rollout_reset` on the device path: resets every env through the open collector and returns the tensors
    `recv_device_tensors` would (valid until the second next step)."""
    import torch

    dev = torch.device("cuda", pool.device)
    got: list = []
    _order_both_ways(pool, dev, lambda: got.append(pool.rollout_reset_device()))
    return _rollout_tensors(pool, got[0][0], got[0][1], dev)


def rollout_step_device(pool: Any, action: Any) -> dict[str, Any]:
    """One collector step with an action tensor [N, ...] on the pool's device: the env step and the collector's kernels
    are enqueued behind torch's current stream -- nothing crosses PCIe -- and the tensors `recv_device_tensors` would
    return come back, ready for the current stream."""
    import torch

    dev = torch.device("cuda", pool.device)
    want = (pool.num_envs, *pool.action_shape)
    if not action.is_contiguous() or action.dtype != _torch_dtype(pool.action_dtype) or action.device != dev \
            or action.numel() != int(np.prod(want)):
        raise RuntimeError(f"rollout_step_device: action must be a contiguous {np.dtype(pool.action_dtype)} tensor of "
                           f"{want} on {dev}")
    got: list = []
    # (the current stream waits for the pool's stream before this returns, so `action` may be dropped right away)
    _order_both_ways(pool, dev, lambda: got.append(pool.rollout_step_device(action.data_ptr())))
    return _rollout_tensors(pool, got[0][0], got[0][1], dev)


def rollout_view_device(pool: Any) -> dict[str, Any]:
    """The collector's buffers as torch tensors that alias them, by name: each obs key [T+1, N, ...], action [T, N, ...],
    reward float32, term, trunc, mask uint8 [T, N].  No copy; valid until the collector is closed or replaced.  Torch's
    current stream is made to wait for the collector's launches so far."""
    import torch

    dev = torch.device("cuda", pool.device)
    ptrs = pool.rollout_view_device()
    _order_both_ways(pool, dev, lambda: None)
    return {name: torch.as_tensor(_DevArray(p, shape, dtype), device=dev)
            for p, (name, dtype, shape) in zip(ptrs, pool.rollout_arrays())}


def rollout_gae_device(pool: Any, values: Any, gamma: float, lam: float, out: Any = None) -> tuple[Any, Any]:
    """`pool.rollout_gae` with `values` float32 [T+1, N] on the pool's device: (advantages, returns) float32 [T, N]
    tensors, written by the GAE kernel.  `out`: a pair of contiguous float32 [T, N] tensors to write into."""
    import torch

    dev = torch.device("cuda", pool.device)
    t, n = pool.rollout_horizon, pool.num_envs
    if values.dtype != torch.float32 or not values.is_contiguous() or tuple(values.shape) != (t + 1, n) \
            or values.device != dev:
        raise ValueError(f"rollout_gae_device: values must be a contiguous float32 tensor of {(t + 1, n)} on {dev}")
    for name, x in (("gamma", gamma), ("lam", lam)):
        if not 0.0 <= float(x) <= 1.0:
            raise ValueError(f"rollout_gae_device: {name} = {x!r} must be a number in [0, 1]")
    if out is None:
        out = (torch.empty((t, n), dtype=torch.float32, device=dev), torch.empty((t, n), dtype=torch.float32, device=dev))
    for o in out:
        if o.dtype != torch.float32 or not o.is_contiguous() or tuple(o.shape) != (t, n) or o.device != dev:
            raise ValueError(f"rollout_gae_device: out must be two contiguous float32 tensors of {(t, n)} on {dev}")
    _order_both_ways(pool, dev, lambda: pool.rollout_gae_device(values.data_ptr(), gamma, lam, out[0].data_ptr(),
                                                                 out[1].data_ptr()))
    return out[0], out[1]


def rollout_episodes_view_device(pool: Any) -> tuple[tuple, Any]:
    """The finished episodes as torch tensors that alias the buffer -- (env_id int32, step int64, ret float64, length
    int32, each [episodes]) -- and the int32 [1] count tensor; rows at and above the count are undefined.  Read-only:
    `pool.rollout_episodes()` drains."""
    import torch

    dev = torch.device("cuda", pool.device)
    ptrs, count = pool.rollout_episodes_view_device()
    n = pool.rollout_capacity
    _order_both_ways(pool, dev, lambda: None)
    dtypes = (np.int32, np.int64, np.float64, np.int32)
    arrays = tuple(torch.as_tensor(_DevArray(p, (n,), d), device=dev) if n else torch.empty(0, device=dev)
                   for p, d in zip(ptrs, dtypes))
    return arrays, torch.as_tensor(_DevArray(count, (1,), np.int32), device=dev)


def rollout_moments_device(pool: Any) -> Any:
    """The moment accumulators as a float64 [3, components] tensor that aliases them: count, sum, sumsq."""
    import torch

    dev = torch.device("cuda", pool.device)
    ptr, comps = pool.rollout_moments_device()
    _order_both_ways(pool, dev, lambda: None)
    return torch.as_tensor(_DevArray(ptr, (3, comps), np.float64), device=dev)


def rollout_collect_device(pool: Any, steps: int = 0) -> None:
    """`pool.rollout_collect` on the device path: `steps` steps (0: the rest of the horizon) of the attached actor are
    enqueued behind torch's current stream and nothing waits; the current stream then waits for the pool's stream."""
    import torch

    _order_both_ways(pool, torch.device("cuda", pool.device), lambda: pool.rollout_collect(steps, wait=False))


def actor_view_device(pool: Any) -> tuple[Any, Any]:
    """(logp float32 [T, N], value float32 [T + 1, N]) of the attached actor as tensors that alias the buffers."""
    import torch

    dev = torch.device("cuda", pool.device)
    logp, value = pool.actor_view_device()
    t, n = pool.rollout_horizon, pool.num_envs
    _order_both_ways(pool, dev, lambda: None)
    return (torch.as_tensor(_DevArray(logp, (t, n), np.float32), device=dev),
            torch.as_tensor(_DevArray(value, (t + 1, n), np.float32), device=dev))


def actor_eval_device(pool: Any, obs: Any, env_ids: Any, step: int) -> tuple[Any, Any, Any]:
    """`pool.actor_eval` on tensors of the pool's device: `obs` one contiguous tensor per obs key (or the tensor, for
    a single key) of the key's dtype with a row per env id, `env_ids` int32 [k] global ids.  Returns (action, logp,
    value) tensors; only enqueued, ordered both ways with torch's current stream."""
    import torch

    dev = torch.device("cuda", pool.device)
    obs = [obs] if isinstance(obs, torch.Tensor) else list(obs)
    keys = pool.rollout_obs_keys()
    k = int(env_ids.numel())
    if env_ids.dtype != torch.int32 or not env_ids.is_contiguous() or env_ids.device != dev or k < 1:
        raise ValueError(f"actor_eval_device: env_ids must be a contiguous int32 tensor on {dev}")
    if len(obs) != len(keys):
        raise ValueError(f"actor_eval_device: {len(obs)} observation tensors for {len(keys)} obs keys")
    for i, o in zip(keys, obs):
        _, dtype, shape = pool.state_keys[i]
        if o.dtype != _torch_dtype(dtype) or not o.is_contiguous() or o.device != dev \
                or o.numel() != k * int(np.prod(shape, dtype=np.int64)):
            raise ValueError(f"actor_eval_device: an observation must be a contiguous {np.dtype(dtype)} tensor of "
                             f"{(k, *shape)} on {dev}")
    action = torch.empty((k, *pool.action_shape), dtype=_torch_dtype(pool.action_dtype), device=dev)
    logp = torch.empty((k,), dtype=torch.float32, device=dev)
    value = torch.empty((k,), dtype=torch.float32, device=dev)
    _order_both_ways(pool, dev, lambda: pool.actor_eval_device([o.data_ptr() for o in obs], env_ids.data_ptr(), k,
                                                               int(step), action.data_ptr(), logp.data_ptr(),
                                                               value.data_ptr()))
    return action, logp, value
