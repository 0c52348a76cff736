"""The device path of `Net.module(kernels=True)` (csrc/pgx_train.hip.h is the contract, csrc/pgx_train.hip the kernels)
and of `ConvNet.module(kernels=True)` (csrc/pgx_conv_train.hip.h, csrc/pgx_conv_train.hip):
`integers(module, x)` and `conv_integers(module, x)` are the twins' `integers` as a `torch.autograd.Function` whose
forward and backward are the training kernels.  The master parameters are quantised in torch on the device, as the twin quantises them, and handed
over as int8 / int32 tensors; nothing goes through the host.  One training handle per (kind, device, sizes) is kept
and grows with the largest row count seen; `release()` frees them all."""
from __future__ import annotations

import ctypes
from typing import Any

from envpool_amd.core import native

MAX_ROWS = 1 << 20
ERR = 2.0 ** -12  # c: the per-layer relative error constant of the backward kernels (derived in the contract header)
CONV_ERR = 2.0 ** -10  # c_conv: the same of the convolutional kernels (derived in csrc/pgx_conv_train.hip.h)
CONV_MAX_POSITIONS = 1 << 22  # rows * H W of a ConvNet


def conv_max_rows(squares: int) -> int:
    return CONV_MAX_POSITIONS // squares

_handles: dict[tuple, "_Handle"] = {}


def check_input(x: Any, max_rows: int = MAX_ROWS, kind: str = "net") -> None:
    """What `kernels=True` refuses on any device: an input that requires grad, and rows outside 1 .. `max_rows`, the
    cap of the kind (2^20 for a Net, 2^22 / (H W) for a ConvNet)."""
    if x.requires_grad:
        raise ValueError(f"{kind}: kernels=True computes no gradient for the input; x must not require grad")
    if not 1 <= int(x.shape[0]) <= max_rows:
        raise ValueError(f"{kind}: rows = {int(x.shape[0])} must be 1 .. {max_rows} with kernels=True")


def input_integers(x: Any) -> Any:
    """x as the contract's input on either path of `kernels=True`: rounded half to even and clamped to 0 .. 127 (NaN:
    0), which leaves what the contract allows as it is, so the kernels and the twin's code see the same numbers."""
    import torch

    if x.is_floating_point():
        x = torch.nan_to_num(torch.round(x.detach()), nan=0.0)
    return torch.clamp(x.to(torch.uint8) if x.dtype == torch.bool else x, 0, 127)


def release() -> None:
    """Frees every cached training handle and its device memory (up to about (2 L + 9) rows D bytes each, for a
    ConvNet that times H W, kept at the largest row count seen); the next `integers` makes a new one.  A backward whose forward came before the call
    repeats that forward."""
    while _handles:
        _handles.popitem()[1].close()


class _Handle:
    """A training handle (epa_net_train_create, or epa_conv_train_create for kind "conv") and the forward whose
    activations it holds (`ticket`)."""

    def __init__(self, kind: str, device: int, sizes: tuple, max_rows: int):
        self.kind, self.max_rows, self.ticket, self._h = kind, max_rows, None, None
        out = ctypes.c_void_p()
        native.check(self.call("create")(device, *sizes, max_rows, ctypes.byref(out)))
        self._h = out

    def call(self, name: str) -> Any:
        return getattr(native.lib(), f"epa_{self.kind}_train_{name}")

    def close(self) -> None:
        h, self._h = self._h, None
        if h is not None:
            self.call("destroy")(h)

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:  # (interpreter shutdown)
            pass


def _handle(kind: str, device: int, sizes: tuple, rows: int) -> _Handle:
    key = (kind, device) + sizes
    h = _handles.get(key)
    if h is None or h.max_rows < rows:
        if h is not None:
            h.close()  # (hipFree waits for the launches that still use the block)
        cap = MAX_ROWS if kind == "net" else conv_max_rows(sizes[0] * sizes[1])
        h = _handles[key] = _Handle(kind, device, sizes, min(cap, max(min(cap, 4096), 1 << (rows - 1).bit_length())))
    return h


def _pointers(tensors: Any) -> Any:
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _forward(h: _Handle, stream: int, sizes: tuple, shifts: list, x8: Any, wq: list, bq: list) -> Any:
    import torch

    actions = sizes[1] if h.kind == "net" else sizes[3]
    p = torch.empty((x8.shape[0], actions + 1), dtype=torch.int32, device=x8.device)
    native.check(h.call("forward_device")(
        h._h, ctypes.c_void_p(stream), x8.shape[0], _pointers(wq), _pointers(bq),
        (ctypes.c_int32 * len(shifts))(*shifts), x8.data_ptr(), p.data_ptr()))
    return p


def _function() -> Any:
    import torch

    class NetIntegers(torch.autograd.Function):
        @staticmethod
        def forward(ctx: Any, x8: Any, kind: str, sizes: tuple, shifts: list, *params: Any) -> Any:
            n = len(params) // 2
            # the twin's quantising: round half to even, the weight clamp (and the contract's bound of a bias)
            wq = [torch.clamp(torch.round(w.detach()), -127, 127).to(torch.int8).contiguous() for w in params[:n]]
            bq = [torch.clamp(torch.round(b.detach()), -2.0 ** 30, 2.0 ** 30).to(torch.int32).contiguous()
                  for b in params[n:]]
            h = _handle(kind, x8.device.index, sizes, x8.shape[0])
            stream = torch.cuda.current_stream(x8.device).cuda_stream
            p = _forward(h, stream, sizes, shifts, x8, wq, bq)
            h.ticket = ctx.ticket = object()
            ctx.kept = (kind, sizes, shifts, x8, wq, bq)
            ctx.like = [(t.shape, t.dtype) for t in params]
            return p.to(torch.float64)

        @staticmethod
        def backward(ctx: Any, dp: Any) -> Any:
            kind, sizes, shifts, x8, wq, bq = ctx.kept
            h = _handle(kind, x8.device.index, sizes, x8.shape[0])
            stream = torch.cuda.current_stream(x8.device).cuda_stream
            if h.ticket is not ctx.ticket:  # another forward has used the handle since: make this one's again
                _forward(h, stream, sizes, shifts, x8, wq, bq)
                h.ticket = ctx.ticket
            dp = dp.to(torch.float32).contiguous()
            dw = [torch.empty(w.shape, dtype=torch.float32, device=x8.device) for w in wq]
            db = [torch.empty(b.shape, dtype=torch.float32, device=x8.device) for b in bq]
            native.check(h.call("backward_device")(
                h._h, ctypes.c_void_p(stream), x8.shape[0], dp.data_ptr(), _pointers(dw), _pointers(db)))
            grads = [g.to(dtype) for g, (_, dtype) in zip(dw + db, ctx.like)]
            return (None, None, None, None) + tuple(grads)

    return NetIntegers


_fn: Any = None


def _apply(kind: str, module: Any, x8: Any, sizes: tuple) -> Any:
    global _fn
    if _fn is None:
        _fn = _function()
    for t in (*module.weights, *module.biases):
        if t.device != x8.device:
            raise ValueError(f"{kind}: a parameter is on {t.device} and x on {x8.device}; move the module to x's "
                             f"device")
    return _fn.apply(x8, kind, sizes, [int(s) for s in module.shifts], *module.weights, *module.biases)


def integers(module: Any, x: Any) -> Any:
    """The head's p of `module` (a `Net.module(kernels=True)`) for x [rows, F] on a ROCm device, as float64
    [rows, A + 1]: x holds integers 0 .. 127 (what PGX observations and the actor's features are; `input_integers`
    makes them of anything else).  The module's parameters are on x's device, or it is a ValueError."""
    import torch

    x8 = input_integers(x).to(torch.uint8).contiguous()
    sizes = (int(x8.shape[1]), module.actions, module.hidden, module.blocks)
    if sizes[0] != module.weights[0].shape[1]:
        raise ValueError(f"net: x has {sizes[0]} components for a net of F = {module.weights[0].shape[1]}")
    return _apply("net", module, x8, sizes)


def conv_integers(module: Any, x: Any) -> Any:
    """The same for a `ConvNet.module(kernels=True)`: x [rows, H W C] (the board as [H, W, C]) on a ROCm device -> the
    head's p as float64 [rows, A + 1]."""
    import torch

    x8 = input_integers(x).to(torch.uint8).contiguous()
    sizes = tuple(module.obs_shape) + (module.actions, module.channels, module.blocks, module.planes)
    if int(x8.shape[1]) != sizes[0] * sizes[1] * sizes[2]:
        raise ValueError(f"conv: x has {int(x8.shape[1])} components for a net of H W C = {sizes[0] * sizes[1] * sizes[2]}")
    return _apply("conv", module, x8, sizes)
