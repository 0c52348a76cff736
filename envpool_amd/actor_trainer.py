"""The PPO trainer of the rollout actor (csrc/ppo_trainer.hip.h is the contract, csrc/ppo_trainer.hip the kernels),
reached as `actor.trainer(...)`: a whole `fit` of a collected horizon on the device -- the collector's GAE, advantage
statistics, epochs of minibatches sampled without replacement and gathered straight out of the collector's buffers,
forward, the clipped-surrogate loss, backward, gradient norm and clipping, SGD with momentum or Adam on float64 masters
(a Box head's sigma among them), re-quantising -- enqueued by one C++ call.

    tr = actor.trainer(device=0, optimizer="adam", lr=3e-2, clip_ratio=0.2, entropy_weight=0.0, max_rows=4096)
    ro.attach(actor, seed=1); ro.reset()
    for it in range(iters):
        ro.collect()
        tr.fit(ro, epochs=4, batch=4096, gamma=0.99, lam=0.95)   # only enqueues
        print(tr.stats()[-1])                                     # the one host wait
        ro.attach(tr.actor(), seed=1); ro.next()
"""
from __future__ import annotations

import ctypes
from typing import Any

import numpy as np

from envpool_amd.actor import BOX, MASKED, Actor
from envpool_amd.core import native
from envpool_amd.pgx.net import Net
from envpool_amd.pgx.trainer import OPTIMIZERS, STAT_ROWS, _number

MASTER, STATE1, STATE2, QUANTISED, GRADIENT, DP, P, STATS, INFO, BATCH = range(10)  # epa_ppo_read's `what`
FEATURES, ACTION, LOGP, ADV, RET, MASK, ADV_STATS, LEGAL = range(8)                 # the parts of BATCH
DTYPE_CODES = {np.dtype(v): k for k, v in native.DTYPES.items()}


def pack_legal(legal: Any, actions: int) -> np.ndarray:
    """uint32 [rows, 4] of bool [rows, H]: bit j of a row in word j // 32; a row without a legal action is all ones."""
    legal = np.asarray(legal, np.bool_).reshape(-1, actions)
    bits = np.zeros((len(legal), 128), np.uint8)
    bits[:, :actions] = legal
    bits[~legal.any(axis=1)] = 1
    return np.packbits(bits, axis=1, bitorder="little").view("<u4").astype(np.uint32)


class ActorTrainer:
    """`actor.trainer(...)`.  The masters start as the actor's integers and sigma, the optimizer state as zeros; the
    actor itself is not changed.  Calls only enqueue (`step` on torch's current stream of the device, `fit` on the
    pool's stream, ordered both ways against it); `stats()`, `read()` and `actor()` wait."""

    def __init__(self, actor: Actor, device: int = 0, optimizer: str = "adam", lr: float = 3e-2,
                 betas: tuple = (0.9, 0.999), eps: float = 1e-8, momentum: float = 0.9, weight_decay: float = 0.0,
                 clip_ratio: float = 0.2, value_weight: float = 0.5, entropy_weight: float = 0.0,
                 normalize_adv: bool = True, train_sigma: bool = True, clip: float = 0.5, seed: int = 0,
                 max_rows: int = 4096):
        self._h = None
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"trainer: optimizer = {optimizer!r} must be one of {sorted(OPTIMIZERS)}")
        if isinstance(max_rows, bool) or int(max_rows) != max_rows or not 1 <= int(max_rows) <= 1 << 22:
            raise ValueError(f"trainer: max_rows = {max_rows} must be an integer in 1 .. 2^22")
        for name, v in (("normalize_adv", normalize_adv), ("train_sigma", train_sigma)):
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError(f"trainer: {name} = {v!r} must be a bool")
        base = native.TrainerOptions(
            OPTIMIZERS[optimizer], 0, _number("lr", lr), _number("momentum", momentum), _number("beta1", betas[0]),
            _number("beta2", betas[1]), _number("eps", eps), _number("weight_decay", weight_decay),
            _number("value_weight", value_weight), _number("clip", clip), int(seed) & (2 ** 64 - 1))
        o = native.PpoOptions(base, _number("clip_ratio", clip_ratio), _number("entropy_weight", entropy_weight),
                              int(normalize_adv), int(train_sigma))
        self._actor, self.device, self.max_rows = actor, int(device), int(max_rows)
        self._layers = len(actor.net.layers)
        self.sigma_layer = 2 * self._layers if actor.kind == BOX and train_sigma else None  # `layer` of the segment
        self._last = 0  # the steps of the last call
        blob = actor.blob()
        out = ctypes.c_void_p()
        native.check(native.lib().epa_ppo_create(self.device, blob.ctypes.data, blob.nbytes, ctypes.byref(o),
                                                 self.max_rows, ctypes.byref(out)))
        self._h = out

    def _open(self) -> Any:
        if self._h is None:
            raise ValueError("trainer: the trainer is closed")
        return self._h

    def close(self) -> None:
        h, self._h = self._h, None
        if h is not None:
            native.lib().epa_ppo_destroy(h)

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:  # (interpreter shutdown)
            pass

    # -- steps -----------------------------------------------------------------------
    def step(self, features: Any, action: Any, logp: Any, adv: Any, ret: Any, mask: Any = None, legal: Any = None) -> None:
        """One step on a minibatch the caller has put together: features uint8 [rows, F] (`actor.features_of`), action
        int32 [rows] (Discrete; MASKED: the flat index) or float32 [rows, H] (Box), logp, adv, ret float32 [rows], mask
        bool [rows] or None -- numpy arrays, or torch tensors on the device (then nothing is copied and nothing waits).
        `adv` is used as given.  A MASKED actor needs `legal`: the rows' legal words uint32 [rows, 4], or bool [rows, H],
        which is packed here before it goes to the device (a row without a legal action: every action)."""
        import torch

        h = self._open()
        a = self._actor
        dev = torch.device("cuda", self.device)
        box = a.kind == BOX
        if (a.kind == MASKED) != (legal is not None):
            raise ValueError("trainer: legal is required for a masked actor (kind 2) and taken by no other")
        if legal is not None:
            legal = legal.cpu().numpy() if hasattr(legal, "cpu") else np.asarray(legal)
            if legal.dtype == np.bool_:
                legal = pack_legal(legal, a.actions)
            legal = np.ascontiguousarray(legal, np.uint32).view(np.int32)  # (torch has no uint32 arithmetic; bits only)
        kept = []
        for name, x, dtype in (("features", features, torch.uint8), ("action", action, torch.float32 if box else torch.int32),
                               ("logp", logp, torch.float32), ("adv", adv, torch.float32), ("ret", ret, torch.float32),
                               ("mask", mask, torch.uint8), ("legal", legal, torch.int32)):
            if x is None:
                kept.append(None)
                continue
            if isinstance(x, np.ndarray):
                x = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
            elif x.device != dev:
                raise ValueError(f"trainer: {name} is on {x.device}; the trainer is on {dev}")
            if x.dtype == torch.bool:
                x = x.view(torch.uint8)
            kept.append(x.to(dtype).contiguous())
        rows = int(kept[2].numel())
        for name, x, n in (("features", kept[0], rows * a.features), ("action", kept[1], rows * (a.actions if box else 1)),
                           ("adv", kept[3], rows), ("ret", kept[4], rows), ("mask", kept[5], rows),
                           ("legal", kept[6], rows * 4)):
            if x is not None and x.numel() != n:
                raise ValueError(f"trainer: {name} has {x.numel()} elements for {rows} rows ({n})")
        stream = torch.cuda.current_stream(dev).cuda_stream
        call = native.lib().epa_ppo_step_legal_device if a.kind == MASKED else native.lib().epa_ppo_step_device
        native.check(call(h, ctypes.c_void_p(stream), rows,
                          *[x.data_ptr() if x is not None else None for x in kept[:7 if a.kind == MASKED else 6]]))
        self._kept = kept  # (until the next call: the launches read them)
        self._last = 1

    def fit(self, ro: Any, epochs: int = 4, batch: int = 4096, gamma: float = 0.99, lam: float = 0.95) -> None:
        """A whole PPO fit of the horizon `ro` (a `RolloutCollector` with an actor attached) has collected: its GAE
        over the stored values, then `epochs` epochs of T N // batch minibatches each, read where the collector's
        buffers lie.  ValueError: no actor attached, a horizon that is not full, another device, an actor of another
        F, H or kind, batch > min(T N, max_rows), a sharded pool."""
        import torch

        from envpool_amd import torch_interop

        h = self._open()
        for name, v in (("epochs", epochs), ("batch", batch)):
            if isinstance(v, bool) or int(v) != v or int(v) < 1:
                raise ValueError(f"trainer: {name} = {v} must be an integer of at least 1")
        pool = ro._open()
        if hasattr(pool, "pools"):
            raise ValueError("trainer: a sharded pool is not supported (one device, one collector)")
        if ro._actor is None:
            raise ValueError("trainer: the collector has no actor (attach one)")
        if pool.device != self.device:
            raise ValueError(f"trainer: the collector's pool is on device {pool.device}, the trainer on {self.device}")
        a = self._actor
        if pool.actor_shape()[:3] != (a.features, a.actions, a.kind):
            raise ValueError(f"trainer: the attached actor has (F, H, kind) = {pool.actor_shape()[:3]}; the trainer's "
                             f"has {(a.features, a.actions, a.kind)}")
        horizon, envs, _, t = pool.rollout_shape()[:4]
        if t < horizon:
            raise ValueError(f"trainer: {t} of {horizon} steps collected; a fit needs the whole horizon")
        if batch > min(horizon * envs, self.max_rows):
            raise ValueError(f"trainer: batch = {batch} must not exceed min(T N = {horizon * envs}, max_rows = "
                             f"{self.max_rows})")
        views = pool.rollout_view_device()
        keys = pool.rollout_obs_keys()
        src = native.PpoSource()
        src.horizon, src.envs, src.n_obs = horizon, envs, len(keys)
        for j, i in enumerate(keys):
            _, dtype, shape = pool.state_keys[i]
            src.obs_dtype[j], src.obs_elems[j] = DTYPE_CODES[np.dtype(dtype)], int(np.prod(shape, dtype=np.int64))
            src.obs[j] = views[j]
        src.action_dtype = DTYPE_CODES[np.dtype(pool.action_dtype)]
        src.action_elems = int(np.prod(pool.action_shape, dtype=np.int64))
        src.action, src.mask, src.logp = views[len(keys)], views[len(keys) + 4], pool.actor_view_device()[0]
        lib = native.lib()
        torch_interop._order_both_ways(pool, torch.device("cuda", pool.device), lambda: native.check(
            lib.epa_ppo_fit_device(h, pool._h, ctypes.c_void_p(pool.stream), ctypes.byref(src), int(epochs), int(batch),
                                   float(np.float32(gamma)), float(np.float32(lam)))))
        self._last = int(epochs) * (horizon * envs // int(batch))

    # -- the way back (host waits) -----------------------------------------------------
    def read(self, what: int, layer: int = 0) -> np.ndarray:
        """`epa_ppo_read`: as `Trainer.read`, with the sigma segment as parameter array `sigma_layer` (MASTER, STATE1,
        STATE2, GRADIENT; QUANTISED: the float32 sigma the loss reads) and BATCH: part `layer` (FEATURES, ACTION, LOGP,
        ADV, RET, MASK, ADV_STATS, and LEGAL uint32 [rows, 4] of a MASKED actor) of the last minibatch a `fit` gathered."""
        h = self._open()
        lib = native.lib()
        a = self._actor
        info = np.zeros(4, np.int64)
        native.check(lib.epa_ppo_read(h, INFO, layer if what <= GRADIENT else 0, info.ctypes.data))
        rows = int(info[2])
        if what <= GRADIENT and layer == self.sigma_layer:
            out = np.empty(a.actions, np.float64 if what <= STATE2 else np.float32)
        elif what <= GRADIENT:
            weight = layer < self._layers
            like = a.net.layers[layer % self._layers][0 if weight else 1]
            dtype = (np.float64 if what <= STATE2 else np.float32 if what == GRADIENT else
                     np.int8 if weight else np.int32)
            out = np.empty(like.shape, dtype)
        elif what in (DP, P):
            out = np.empty((rows, a.actions + 1), np.float32 if what == DP else np.int32)
        elif what == STATS:
            out = np.empty((int(layer), 8), np.float64)
        else:
            box = a.kind == BOX
            shapes = {FEATURES: ((rows, a.features), np.uint8), LOGP: ((rows,), np.float32), ADV: ((rows,), np.float32),
                      ACTION: ((rows, a.actions) if box else (rows,), np.float32 if box else np.int32),
                      RET: ((rows,), np.float32), MASK: ((rows,), np.uint8), ADV_STATS: ((3,), np.float64)}
            if a.kind == MASKED:
                shapes[LEGAL] = ((rows, 4), np.uint32)
            if layer not in shapes:
                raise ValueError(f"trainer: a minibatch has parts 0 .. {len(shapes) - 1}, not {layer}")
            out = np.empty(*shapes[layer])
        if out.size:
            native.check(lib.epa_ppo_read(h, int(what), int(layer), out.ctypes.data))
        return out

    def stats(self) -> np.ndarray:
        """float64 [steps, 8] of the last call (its last 4096 steps): policy loss, value loss, entropy, approximate KL,
        clip fraction, the global gradient norm before clipping, the unmasked rows, the rows."""
        return self.read(STATS, min(self._last, STAT_ROWS))

    def actor(self) -> Actor:
        """A new `Actor` of the quantised arrays and the trained sigma as they stand; lo, scale, low and high are the
        old ones.  What `ro.attach` takes."""
        n, a = self._layers, self._actor
        layers = [(self.read(QUANTISED, i), self.read(QUANTISED, n + i), s) for i, (_, _, s) in enumerate(a.net.layers)]
        t = a.net
        net = Net(t.obs_shape, t.actions, t.hidden, t.blocks, layers, t.scale_p, t.scale_v)
        sigma = self.read(QUANTISED, self.sigma_layer) if self.sigma_layer is not None else a.sigma
        masked = dict(mask0=a.mask0, nvec=a.nvec[:a.components]) if a.kind == MASKED else {}
        return Actor(net, a.kind, a.lo, a.scale, sigma, a.low, a.high, **masked)
