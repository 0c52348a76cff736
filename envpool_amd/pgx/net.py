"""The PGX built-in network (csrc/pgx_net.hip.h is the contract): an NNUE-style policy-value network in exact integer
arithmetic, evaluated on the device by one kernel (csrc/pgx_net.hip), as the evaluator of the guided and Gumbel
sessions.

    net = Net.random((8, 8, 2), 65, hidden=128, blocks=2, seed=0)        # or Net.load("othello.npz")
    while playing:
        result = env.gumbel_search(ids, simulations=32, batch=16).run(net)   # a whole round enqueued from C++
        env.step(result.action, ids)

`search.run(net)` makes the round without Python between its launches; `net.bind(env)` gives a plain callable with the
`evaluate` signature (numpy in and out, or torch tensors on the pool's device) for every entry point that takes one.
`Net.module()` is a torch twin that computes the same integers in float64 with straight-through gradients, and
`Net.from_module` comes back: the format is trainable."""
from __future__ import annotations

import ctypes
from typing import Any, Sequence

import numpy as np

from envpool_amd.core import native

MAGIC = 0x4E584750  # "PGXN"
VERSION = 1
HEADER_BYTES = 32
MIN_WIDTH, MAX_WIDTH = 32, 512
MAX_BLOCKS, MAX_SHIFT, MAX_INPUTS, MAX_ACTIONS, MAX_BIAS = 8, 24, 512, 127, 1 << 30
LOGITS, PRIORS = 0, 1


def _check_sizes(f: int, a: int, d: int, blocks: int) -> None:
    if not 1 <= f <= MAX_INPUTS:
        raise ValueError(f"net: F = {f} must be 1 .. {MAX_INPUTS}")
    if not 1 <= a <= MAX_ACTIONS:
        raise ValueError(f"net: A = {a} must be 1 .. {MAX_ACTIONS}")
    if not MIN_WIDTH <= d <= MAX_WIDTH or d % 32:
        raise ValueError(f"net: D = {d} must be a multiple of 32 in {MIN_WIDTH} .. {MAX_WIDTH}")
    if not 0 <= blocks <= MAX_BLOCKS:
        raise ValueError(f"net: L = {blocks} must be 0 .. {MAX_BLOCKS}")


class Net:
    """`layers`: the 2 * blocks + 2 layers in the blob's order -- trunk, the two of every block, head -- each a tuple
    (weights int8 [N, K], bias int32 [N], shift int); the trunk is [hidden, F], a block's layers [hidden, hidden], the
    head [actions + 1, hidden] with shift 0.  Everything the contract bounds is checked here (ValueError)."""

    _is_epa_net = True

    def __init__(self, obs_shape: Sequence[int], actions: int, hidden: int, blocks: int, layers: Sequence[tuple],
                 scale_p: float, scale_v: float):
        self.obs_shape = tuple(int(x) for x in obs_shape)
        self.inputs = int(np.prod(self.obs_shape))
        self.actions, self.hidden, self.blocks = int(actions), int(hidden), int(blocks)
        _check_sizes(self.inputs, self.actions, self.hidden, self.blocks)
        if len(layers) != 2 * self.blocks + 2:
            raise ValueError(f"net: {len(layers)} layers for L = {self.blocks} (2 L + 2 = {2 * self.blocks + 2})")
        self.scale_p, self.scale_v = float(np.float32(scale_p)), float(np.float32(scale_v))
        for name, s in (("scale_p", self.scale_p), ("scale_v", self.scale_v)):
            if not 0.0 < s <= 1e20:
                raise ValueError(f"net: {name} must be finite, above 0 and at most 1e20")
        self.layers = []
        for i, (w, b, shift) in enumerate(layers):
            head = i == len(layers) - 1
            n, k = (self.actions + 1 if head else self.hidden), (self.inputs if i == 0 else self.hidden)
            w, b, shift = np.asarray(w), np.asarray(b), int(shift)
            if w.shape != (n, k) or b.shape != (n,):
                raise ValueError(f"net: layer {i}: weights {w.shape} and bias {b.shape} must be ({n}, {k}) and ({n},)")
            if not 0 <= shift <= (0 if head else MAX_SHIFT):
                raise ValueError(f"net: layer {i}: shift = {shift} must be 0 .. {0 if head else MAX_SHIFT}")
            if np.any(w != np.rint(w)) or np.any(np.abs(w.astype(np.int64)) > 127):
                bad = "a weight of -128" if np.any(w == -128) else "a weight outside -127 .. 127"
                raise ValueError(f"net: layer {i}: {bad} (weights are -127 .. 127)")
            if np.any(np.abs(b.astype(np.int64)) > MAX_BIAS):
                raise ValueError(f"net: layer {i}: a bias of {int(b[np.argmax(np.abs(b.astype(np.int64)))])} is past "
                                 f"2^30 in magnitude")
            self.layers.append((np.ascontiguousarray(w, np.int8), np.ascontiguousarray(b, np.int32), shift))
        self._handles: dict[int, Any] = {}
        self._bound: Any = None

    # -- the blob ------------------------------------------------------------------
    def blob(self) -> np.ndarray:
        """The network as the C ABI takes it (include/envpool_amd.h): uint8, 4-byte aligned."""
        parts = [np.array([MAGIC, VERSION, self.inputs, self.actions, self.hidden, self.blocks], "<u4").tobytes(),
                 np.array([self.scale_p, self.scale_v], "<f4").tobytes()]
        for w, b, shift in self.layers:
            raw = w.tobytes()
            parts += [raw, b"\0" * (-len(raw) % 4), b.astype("<i4").tobytes(), np.array([shift], "<i4").tobytes()]
        return np.frombuffer(b"".join(parts), np.uint8).copy()

    @classmethod
    def from_blob(cls, blob: Any, obs_shape: Any = None) -> "Net":
        blob = np.ascontiguousarray(blob, np.uint8)
        if blob.nbytes < HEADER_BYTES:
            raise ValueError(f"net: a blob of {blob.nbytes} bytes is shorter than a header")
        magic, version, f, a, d, blocks = (int(x) for x in blob[:24].view("<i4"))
        if magic != MAGIC:
            raise ValueError("net: the blob does not begin with the magic PGXN")
        if version != VERSION:
            raise ValueError(f"net: version = {version} must be {VERSION}")
        _check_sizes(f, a, d, blocks)
        scale_p, scale_v = (float(x) for x in blob[24:32].view("<f4"))
        at, layers = HEADER_BYTES, []
        for i in range(2 * blocks + 2):
            n, k = (a + 1 if i == 2 * blocks + 1 else d), (f if i == 0 else d)
            need = at + (n * k + 3) // 4 * 4 + 4 * n + 4
            if blob.nbytes < need:
                raise ValueError(f"net: a blob of {blob.nbytes} bytes ends inside layer {i}")
            w = blob[at:at + n * k].view(np.int8).reshape(n, k)
            at += (n * k + 3) // 4 * 4
            b = blob[at:at + 4 * n].view("<i4")
            at += 4 * n
            layers.append((w, b, int(blob[at:at + 4].view("<i4")[0])))
            at += 4
        if at != blob.nbytes:
            raise ValueError(f"net: a blob of {blob.nbytes} bytes for a network of {at} bytes")
        return cls(obs_shape if obs_shape is not None else (f,), a, d, blocks, layers, scale_p, scale_v)

    def save(self, path: str) -> None:
        arrays = {"obs_shape": np.array(self.obs_shape, np.int32), "actions": np.int32(self.actions),
                  "hidden": np.int32(self.hidden), "blocks": np.int32(self.blocks),
                  "scale": np.array([self.scale_p, self.scale_v], np.float32),
                  "shift": np.array([s for _, _, s in self.layers], np.int32)}
        for i, (w, b, _) in enumerate(self.layers):
            arrays[f"w{i}"], arrays[f"b{i}"] = w, b
        with open(path, "wb") as f:  # (np.savez would add ".npz" to a bare name)
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path: str) -> "Net":
        with np.load(path) as z:
            blocks = int(z["blocks"])
            layers = [(z[f"w{i}"], z[f"b{i}"], int(z["shift"][i])) for i in range(2 * blocks + 2)]
            return cls(z["obs_shape"], int(z["actions"]), int(z["hidden"]), blocks, layers, float(z["scale"][0]),
                       float(z["scale"][1]))

    @classmethod
    def random(cls, obs_shape: Sequence[int], actions: int, hidden: int, blocks: int, seed: int = 0,
               shift_delta: int = 0) -> "Net":
        """A network for tests and smoke runs from numpy's PCG64(seed): weights uniform in -127 .. 127, biases uniform
        in -1024 .. 1024, shifts that keep the activations spread over 0 .. 127 for inputs of density 1/4
        (`shift_delta` is added to every shift)."""
        rng = np.random.Generator(np.random.PCG64(seed))
        f = int(np.prod(tuple(obs_shape)))
        s_in = int(round(np.log2(73.0 * np.sqrt(f / 4.0) / 32.0)))
        s_hid = int(round(np.log2(73.0 * np.sqrt(hidden) * 40.0 / 32.0)))
        layers = []
        for i in range(2 * blocks + 2):
            head = i == 2 * blocks + 1
            n, k = (actions + 1 if head else hidden), (f if i == 0 else hidden)
            w = rng.integers(-127, 128, size=(n, k)).astype(np.int8)
            b = rng.integers(-1024, 1025, size=n).astype(np.int32)
            shift = 0 if head else min(MAX_SHIFT, max(0, (s_in if i == 0 else s_hid) + shift_delta))
            layers.append((w, b, shift))
        spread = 73.0 * np.sqrt(hidden) * 40.0  # about the deviation of the head's integers
        return cls(obs_shape, actions, hidden, blocks, layers, 4.0 / spread, 1.0 / spread)

    # -- the device ----------------------------------------------------------------
    def _handle(self, device: int) -> Any:
        """The net on `device` (epa_net_create), uploaded on first use."""
        h = self._handles.get(int(device))
        if h is None:
            blob = self.blob()
            out = ctypes.c_void_p()
            native.check(native.lib().epa_net_create(int(device), blob.ctypes.data, blob.nbytes, ctypes.byref(out)))
            h = self._handles[int(device)] = out
        return h

    def close(self) -> None:
        """Releases the device copies (also done when the object goes)."""
        handles, self._handles = self._handles, {}
        for h in handles.values():
            native.lib().epa_net_destroy(h)

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:  # (interpreter shutdown)
            pass

    def bind(self, env: Any, priors: bool = False) -> Any:
        """A callable `evaluate(obs, mask, status) -> (policy, values)` on `env` (an env of a PGX family, or its
        device pool): numpy arrays in and out, or torch tensors on the pool's device (only enqueued, ordered both ways
        against torch's current stream).  `priors`: the softmax over the legal actions, what a PUCT session takes;
        otherwise logits, what a Gumbel session takes."""
        pool = env._guided() if hasattr(env, "_guided") else env

        def evaluate(obs: Any, mask: Any, status: Any) -> tuple[Any, Any]:
            return self._evaluate(pool, obs, mask, status, priors)

        return evaluate

    def _evaluate(self, pool: Any, obs: Any, mask: Any, status: Any, priors: bool) -> tuple[Any, Any]:
        if isinstance(obs, np.ndarray):
            return pool.net_eval(self, obs, mask, status, priors)
        import torch

        from envpool_amd import torch_interop

        dev = torch.device("cuda", pool.device)
        rows, a = int(status.numel()), self.actions
        for name, t, n in (("obs", obs, rows * self.inputs), ("mask", mask, rows * a), ("status", status, rows)):
            if t.device != dev or not t.is_contiguous() or t.element_size() != 1 or t.numel() != n:
                raise ValueError(f"net: {name} must be a contiguous one-byte tensor of {n} elements on {dev}")
        policy = torch.empty((rows, a), dtype=torch.float32, device=dev)
        value = torch.empty((rows,), dtype=torch.float32, device=dev)
        torch_interop._order_both_ways(pool, dev, lambda: pool.net_eval_device(
            self, rows, priors, obs.data_ptr(), mask.data_ptr(), status.data_ptr(), policy.data_ptr(),
            value.data_ptr()))
        return policy, value

    # -- the torch twin ------------------------------------------------------------
    def module(self) -> Any:
        """A `torch.nn.Module` with this net's numbers as float64 parameters: `forward(x [rows, F]) -> (logits float32
        [rows, A], value float32 [rows])` with the contract's bits, `integers(x)` the head's p as float64; rounding
        passes gradients straight through."""
        return _make_module(self)

    @classmethod
    def from_module(cls, m: Any) -> "Net":
        layers = [(np.clip(np.rint(w.detach().numpy()), -127, 127).astype(np.int8),
                   np.clip(np.rint(b.detach().numpy()), -MAX_BIAS, MAX_BIAS).astype(np.int32), int(s))
                  for w, b, s in zip(m.weights, m.biases, m.shifts)]
        return cls(m.obs_shape, m.actions, m.hidden, m.blocks, layers, m.scale_p, m.scale_v)


def _make_module(net: Net) -> Any:
    import torch

    class NetModule(torch.nn.Module):
        def __init__(self) -> None:
            super().__init__()
            self.obs_shape, self.actions, self.hidden, self.blocks = net.obs_shape, net.actions, net.hidden, net.blocks
            self.scale_p, self.scale_v = net.scale_p, net.scale_v
            self.shifts = [s for _, _, s in net.layers]
            self.weights = torch.nn.ParameterList(
                [torch.nn.Parameter(torch.tensor(w.astype(np.float64))) for w, _, _ in net.layers])
            self.biases = torch.nn.ParameterList(
                [torch.nn.Parameter(torch.tensor(b.astype(np.float64))) for _, b, _ in net.layers])

        @staticmethod
        def _ste(x: Any, q: Any) -> Any:  # the value of q, the gradient of x
            return x + (q - x).detach()

        def _layer(self, i: int, x: Any) -> Any:
            w, b = self.weights[i], self.biases[i]
            w = self._ste(w, torch.clamp(torch.round(w), -127, 127))
            b = self._ste(b, torch.round(b))
            z = x @ w.t() + b
            s = self.shifts[i]
            if s:
                z = self._ste(z / 2.0 ** s, torch.floor((z + 2.0 ** (s - 1)) / 2.0 ** s))
            return z

        def integers(self, x: Any) -> Any:
            x = x.reshape(x.shape[0], -1).to(torch.float64)
            h = torch.clamp(self._layer(0, x), 0, 127)
            for l in range(self.blocks):
                t = torch.clamp(self._layer(1 + 2 * l, h), 0, 127)
                h = torch.clamp(self._layer(2 + 2 * l, t) + h, 0, 127)
            return self._layer(2 * self.blocks + 1, h)

        def forward(self, x: Any) -> tuple[Any, Any]:
            p = self.integers(x).to(torch.float32)
            logits = p[:, :self.actions] * torch.tensor(self.scale_p, dtype=torch.float32)
            value = torch.clamp(p[:, self.actions] * torch.tensor(self.scale_v, dtype=torch.float32), -1.0, 1.0)
            return logits, value

    return NetModule()
