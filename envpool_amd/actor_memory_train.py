"""The device path of `ActorModule.unroll(..., kernels=True)` of a memory actor (csrc/actor_memory_train.hip.h is the
contract, csrc/actor_memory_train.hip the kernels): `unroll_integers(module, x8, h0, mask)` is the cell's unroll and
the trunk's `integers` as ONE `torch.autograd.Function` whose forward and backward are the training kernels -- the
cell's over the whole horizon (epa_cell_train_*), the trunk's (epa_net_train_*) and the trunk's input gradient between
them.  The master parameters are quantised in torch on the device, as the twin quantises them; nothing goes through
the host.  One cell handle per (device, F, M, kind) is kept beside the trunk's (pgx/train.py) and grows with the
largest T N seen; `release()` frees both kinds."""
from __future__ import annotations

import ctypes
from typing import Any

from envpool_amd.core import native
from envpool_amd.pgx import train

MAX_ROWS = train.MAX_ROWS  # T N
ERR = 2.0 ** -12 + 2.0 ** -16 + 2.0 ** -20  # kCellTrainErr: per step of depth (derived in the contract header)

_handles: dict[tuple, "_Handle"] = {}


def depth(blocks: int, horizon: int) -> int:
    """CellTrainDepth: what a gradient of the cell, or dh0, has passed; trunk layer i has 2 L + 2 - i as before."""
    return 2 * blocks + 3 + horizon


def release() -> None:
    """Frees every cached cell handle and the trunk handles of `pgx.train` (about T N (11 M + F) bytes each at the
    largest T N seen); the next `unroll(kernels=True)` makes new ones."""
    while _handles:
        _handles.popitem()[1].close()
    train.release()


class _Handle(train._Handle):
    """A cell handle (epa_cell_train_create) and the forward whose saved bytes it holds (`ticket`)."""

    def __init__(self, device: int, sizes: tuple, max_rows: int):
        super().__init__("cell", device, sizes, max_rows)


def _handle(device: int, sizes: tuple, rows: int) -> _Handle:
    key = (device,) + sizes
    h = _handles.get(key)
    if h is None or h.max_rows < rows:
        if h is not None:
            h.close()  # (hipFree waits for the launches that still use the block)
        h = _handles[key] = _Handle(device, sizes, min(MAX_ROWS, max(4096, 1 << (rows - 1).bit_length())))
    return h


def _quantise(weights: Any, biases: Any) -> tuple[list, list]:
    import torch

    # the twin's quantising: round half to even, the weight clamp (and the contract's bound of a bias)
    wq = [torch.clamp(torch.round(w.detach()), -127, 127).to(torch.int8).contiguous() for w in weights]
    bq = [torch.clamp(torch.round(b.detach()), -2.0 ** 30, 2.0 ** 30).to(torch.int32).contiguous() for b in biases]
    return wq, bq


def _forward(k: dict) -> tuple[Any, Any]:
    """Both forwards of the kept call `k`: (p int32 [T N, A + 1], h uint8 [N, M]); the handles then hold this call."""
    import torch

    x8, (t, n) = k["x8"], k["shape"]
    stream = torch.cuda.current_stream(x8.device).cuda_stream
    cell = _handle(x8.device.index, k["cell_sizes"], t * n)
    net = train._handle("net", x8.device.index, k["net_sizes"], t * n)
    m = k["cell_sizes"][1]
    hp = torch.empty((t * n, m), dtype=torch.uint8, device=x8.device)
    h = torch.empty((n, m), dtype=torch.uint8, device=x8.device)
    native.check(cell.call("forward_device")(
        cell._h, ctypes.c_void_p(stream), t, n, train._pointers(k["cell_wq"]), train._pointers(k["cell_bq"]),
        (ctypes.c_int32 * 2)(*k["cell_shifts"]), x8.data_ptr(), k["h8"].data_ptr(), k["mask8"].data_ptr(),
        hp.data_ptr(), h.data_ptr()))
    p = train._forward(net, stream, k["net_sizes"], k["net_shifts"], hp, k["net_wq"], k["net_bq"])
    cell.ticket = net.ticket = k["ticket"]
    return p, h


def _function() -> Any:
    import torch

    class CellUnroll(torch.autograd.Function):
        @staticmethod
        def forward(ctx: Any, h0: Any, kept: dict, *params: Any) -> Any:
            layers = (len(params) - 4) // 2
            kept["cell_wq"], kept["cell_bq"] = _quantise(params[0:2], params[2:4])
            kept["net_wq"], kept["net_bq"] = _quantise(params[4:4 + layers], params[4 + layers:])
            kept["h8"] = train.input_integers(h0).to(torch.uint8).contiguous()
            kept["ticket"] = object()
            p, h = _forward(kept)
            ctx.kept = kept
            ctx.like = [t.dtype for t in (h0,) + params]
            return p.to(torch.float64), h.to(torch.float64)

        @staticmethod
        def backward(ctx: Any, dp: Any, dh: Any) -> Any:
            k = ctx.kept
            x8, (t, n) = k["x8"], k["shape"]
            dev, (f, m, _) = x8.device, k["cell_sizes"]
            stream = torch.cuda.current_stream(dev).cuda_stream
            cell = _handle(dev.index, k["cell_sizes"], t * n)
            net = train._handle("net", dev.index, k["net_sizes"], t * n)
            if cell.ticket is not k["ticket"] or net.ticket is not k["ticket"]:
                _forward(k)  # another forward has used a handle since: make this one's again
            dp = dp.to(torch.float32).contiguous()
            dw = [torch.empty(w.shape, dtype=torch.float32, device=dev) for w in k["net_wq"]]
            db = [torch.empty(b.shape, dtype=torch.float32, device=dev) for b in k["net_bq"]]
            native.check(net.call("backward_device")(
                net._h, ctypes.c_void_p(stream), t * n, dp.data_ptr(), train._pointers(dw), train._pointers(db)))
            dhp = torch.empty((t * n, m), dtype=torch.float32, device=dev)
            native.check(net.call("input_grad_device")(net._h, ctypes.c_void_p(stream), t * n, dhp.data_ptr()))
            dh = None if dh is None else dh.to(torch.float32).contiguous()
            cw = torch.empty((2, m, f + m), dtype=torch.float32, device=dev)
            cb = torch.empty((2, m), dtype=torch.float32, device=dev)
            dh0 = torch.empty((n, m), dtype=torch.float32, device=dev)
            native.check(cell.call("backward_device")(
                cell._h, ctypes.c_void_p(stream), t, n, dhp.data_ptr(), None if dh is None else dh.data_ptr(),
                cw.data_ptr(), cb.data_ptr(), dh0.data_ptr()))
            grads = [dh0, cw[0], cw[1], cb[0], cb[1]] + dw + db
            return (grads[0].to(ctx.like[0]), None) + tuple(g.to(d) for g, d in zip(grads[1:], ctx.like[1:]))

    return CellUnroll


_fn: Any = None


def unroll_integers(module: Any, x8: Any, h0: Any, mask: Any) -> tuple[Any, Any]:
    """(p float64 [T N, A + 1], h float64 [N, M]) of the feature bytes x8 uint8 [T, N, F], the states h0 [N, M] and
    mask [T, N] on a ROCm device: the trunk's integers of every slot and the state after the last one.  The module's
    parameters are on x8's device, or it is a ValueError."""
    global _fn
    import torch

    if _fn is None:
        _fn = _function()
    net = module.net
    params = (*module.cell_weights, *module.cell_biases, *net.weights, *net.biases)
    for p in (*params, h0, mask):
        if p.device != x8.device:
            raise ValueError(f"actor: a parameter, h0 or mask is on {p.device} and obs on {x8.device}; move the module "
                             f"to obs's device")
    t, n, f = (int(s) for s in x8.shape)
    if not (t >= 1 and n >= 1 and t * n <= MAX_ROWS):
        raise ValueError(f"actor: T N = {t * n} must be 1 .. {MAX_ROWS} with kernels=True")
    kept = dict(x8=x8.contiguous(), shape=(t, n), mask8=(mask != 0).to(torch.uint8).contiguous(),
                cell_sizes=(f, module.memory, module.kind), cell_shifts=[int(s) for s in module.cell_shifts],
                net_sizes=(module.memory, net.actions, net.hidden, net.blocks), net_shifts=[int(s) for s in net.shifts])
    return _fn.apply(h0, kept, *params)
