"""The trainer of the built-in nets (csrc/pgx_trainer.hip.h is the contract, csrc/pgx_trainer.hip the kernels), reached
as `net.trainer(...)`: a whole AlphaZero training step on the device -- minibatch gather, forward, loss, backward,
gradient norm and clipping, SGD with momentum or Adam on float64 masters, re-quantising -- enqueued by one C++ call per
step, or one per `steps` steps.

    tr = net.trainer(device=0, optimizer="sgd", lr=1.0, momentum=0.9, max_rows=4096)
    tr.fit(rec, batch=4096, steps=200)      # minibatches straight out of the recorder's sample arrays
    print(tr.stats()[-1])                   # policy loss, value loss, gradient norm, rows: the one host wait
    net = tr.net()                          # a new Net / ConvNet of the quantised arrays, for search.run(net)
"""
from __future__ import annotations

import ctypes
from typing import Any

import numpy as np

from envpool_amd.core import native

OPTIMIZERS = {"sgd": 0, "adam": 1}
STAT_ROWS = 4096  # kTrainerStatRows: the statistics rows a handle keeps
MASTER, STATE1, STATE2, QUANTISED, GRADIENT, DP, P, STATS, INFO = range(9)  # epa_trainer_read's `what`


def _number(name: str, v: Any) -> float:
    v = float(v)
    if not np.isfinite(v) or v < 0.0:
        raise ValueError(f"trainer: {name} = {v} must be finite and not negative")
    return v


class Trainer:
    """`net.trainer(...)`.  The masters start as the net's integers, the optimizer state as zeros; the net itself is
    not changed.  Calls only enqueue (on torch's current stream of the device; `fit(rec)` on the pool's stream, ordered
    both ways against it); `stats()`, `read()` and `net()` wait."""

    def __init__(self, net: Any, device: int = 0, optimizer: str = "sgd", lr: float = 1.0, momentum: float = 0.9,
                 weight_decay: float = 0.0, value_weight: float = 1.0, clip: float = 0.0, seed: int = 0,
                 max_rows: int = 4096, betas: tuple = (0.9, 0.999), eps: float = 1e-8):
        self._h = None
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"trainer: optimizer = {optimizer!r} must be one of {sorted(OPTIMIZERS)}")
        if isinstance(max_rows, bool) or int(max_rows) != max_rows or int(max_rows) < 1:
            raise ValueError(f"trainer: max_rows = {max_rows} must be an integer of at least 1")
        o = native.TrainerOptions(
            OPTIMIZERS[optimizer], 0, _number("lr", lr), _number("momentum", momentum), _number("beta1", betas[0]),
            _number("beta2", betas[1]), _number("eps", eps), _number("weight_decay", weight_decay),
            _number("value_weight", value_weight), _number("clip", clip), int(seed) & (2 ** 64 - 1))
        self._net, self.device, self.max_rows = net, int(device), int(max_rows)
        self._layers = len(net.layers)
        self._last = 0  # the steps of the last call
        blob = net.blob()
        out = ctypes.c_void_p()
        native.check(native.lib().epa_trainer_create(self.device, blob.ctypes.data, blob.nbytes, ctypes.byref(o),
                                                     self.max_rows, ctypes.byref(out)))
        self._h = out

    def _open(self) -> Any:
        if self._h is None:
            raise ValueError("trainer: the trainer is closed")
        return self._h

    def close(self) -> None:
        h, self._h = self._h, None
        if h is not None:
            native.lib().epa_trainer_destroy(h)

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:  # (interpreter shutdown)
            pass

    # -- steps -----------------------------------------------------------------------
    def _device_rows(self, obs: Any, mask: Any, policy: Any, value: Any) -> tuple:
        """The four arrays as contiguous torch tensors on the device: bytes, bytes, float32, float32."""
        import torch

        dev = torch.device("cuda", self.device)
        out = []
        for name, x, dtype in (("obs", obs, torch.uint8), ("mask", mask, torch.uint8), ("policy", policy, torch.float32),
                               ("value", value, torch.float32)):
            if isinstance(x, np.ndarray):
                x = torch.from_numpy(np.ascontiguousarray(x, np.uint8 if dtype == torch.uint8 else np.float32)).to(dev)
            elif x.device != dev:
                raise ValueError(f"trainer: {name} is on {x.device}; the trainer is on {dev}")
            if x.dtype == torch.bool:
                x = x.view(torch.uint8)
            out.append(x.to(dtype).contiguous())
        rows, a = int(out[3].numel()), self._net.actions
        for name, x, n in (("obs", out[0], rows * self._net.inputs), ("mask", out[1], rows * a),
                           ("policy", out[2], rows * a)):
            if x.numel() != n:
                raise ValueError(f"trainer: {name} has {x.numel()} elements for {rows} rows ({n})")
        return tuple(out)

    def step(self, obs: Any, mask: Any, policy: Any, value: Any) -> None:
        """One step on a minibatch: obs [rows, F] (bool or bytes 0 / 1), mask [rows, A], policy float32 [rows, A], value
        float32 [rows] -- numpy arrays, or torch tensors on the device (then nothing is copied and nothing waits)."""
        import torch

        h = self._open()
        o, m, p, v = self._device_rows(obs, mask, policy, value)
        stream = torch.cuda.current_stream(o.device).cuda_stream
        native.check(native.lib().epa_trainer_step_device(h, ctypes.c_void_p(stream), int(v.numel()), o.data_ptr(),
                                                          m.data_ptr(), p.data_ptr(), v.data_ptr()))
        self._kept = (o, m, p, v)  # (until the next call: the launches read them)
        self._last = 1

    def fit(self, source: Any, batch: int = 4096, steps: int = 1) -> None:
        """`steps` steps of `batch` rows each, sampled with replacement (the contract's index hash of seed, step and
        row).  `source`: a pool's `Recorder` -- its sample arrays on the device, the count read once, ordered after the
        pool's stream and the pool's later calls after it -- or a `Samples`, uploaded once."""
        import torch

        h = self._open()
        for name, v in (("batch", batch), ("steps", steps)):
            if isinstance(v, bool) or int(v) != v:
                raise ValueError(f"trainer: {name} = {v} must be an integer")
        lib = native.lib()
        if hasattr(source, "drain"):  # a Recorder
            from envpool_amd import torch_interop

            pool = source._open()
            count = len(source)
            arrays, _ = pool.record_view_device()
            ptrs = (ctypes.c_void_p * 4)(*arrays[:4])
            dev = torch.device("cuda", pool.device)
            if pool.device != self.device:
                raise ValueError(f"trainer: the recorder's pool is on device {pool.device}, the trainer on {self.device}")
            torch_interop._order_both_ways(pool, dev, lambda: native.check(lib.epa_trainer_fit_device(
                h, ctypes.c_void_p(pool.stream), ptrs, count, int(batch), int(steps))))
        else:
            kept = self._device_rows(source.obs, source.mask, source.policy, source.value)
            ptrs = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in kept])
            stream = torch.cuda.current_stream(kept[0].device).cuda_stream
            native.check(lib.epa_trainer_fit_device(h, ctypes.c_void_p(stream), ptrs, int(kept[3].numel()), int(batch),
                                                    int(steps)))
            self._kept = kept
        self._last = int(steps)

    # -- the way back (host waits) -----------------------------------------------------
    def read(self, what: int, layer: int = 0) -> np.ndarray:
        """`epa_trainer_read`: MASTER, STATE1, STATE2, QUANTISED or GRADIENT of parameter array `layer` (the layers'
        weights in the blob's order, then their biases) in the array's shape; DP / P of the last step [rows, A + 1];
        STATS: the last `layer` statistics rows."""
        h = self._open()
        lib = native.lib()
        info = np.zeros(4, np.int64)
        native.check(lib.epa_trainer_read(h, INFO, layer if what <= GRADIENT else 0, info.ctypes.data))
        if what <= GRADIENT:
            weight = layer < self._layers
            like = self._net.layers[layer % self._layers][0 if weight else 1]
            dtype = (np.float64 if what <= STATE2 else np.float32 if what == GRADIENT else
                     np.int8 if weight else np.int32)
            out = np.empty(like.shape, dtype)
        elif what in (DP, P):
            out = np.empty((int(info[2]), self._net.actions + 1), np.float32 if what == DP else np.int32)
        else:
            out = np.empty((int(layer), 4), np.float64)
        if out.size:
            native.check(lib.epa_trainer_read(h, int(what), int(layer), out.ctypes.data))
        return out

    def stats(self) -> np.ndarray:
        """float64 [steps, 4] of the last call (its last 4096 steps): policy loss and value loss per row, the global
        gradient norm before clipping, the rows."""
        return self.read(STATS, min(self._last, STAT_ROWS))

    def net(self) -> Any:
        """A new Net / ConvNet of the quantised arrays as they stand: what `search.run(net)` takes."""
        n = self._layers
        layers = [(self.read(QUANTISED, i), self.read(QUANTISED, n + i), s) for i, (_, _, s) in enumerate(self._net.layers)]
        t = self._net
        if hasattr(t, "planes"):
            return type(t)(t.obs_shape, t.actions, t.channels, t.blocks, t.planes, layers, t.scale_p, t.scale_v)
        return type(t)(t.obs_shape, t.actions, t.hidden, t.blocks, layers, t.scale_p, t.scale_v)
