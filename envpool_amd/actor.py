"""The rollout actor (csrc/actor.hip.h is the contract): a built-in actor-critic in exact integer arithmetic for the
pools with one row per env, evaluated on the device by the int8 matrix-core kernel of the PGX network between two small
kernels of its own, so that a rollout collector plays whole horizons from C++.

    ro = env.rollout(horizon=128, episodes=1 << 16, moments=True)
    actor = Actor.random(env, hidden=64, blocks=1, seed=0)          # or Actor.load("cartpole.npz")
    ro.attach(actor, seed=1)
    ro.reset()
    ro.collect()                                                     # 128 steps, no Python in between
    b = ro.batch(); adv, ret = ro.gae(); ro.next()                   # b.logp, b.value; the stored values

The observation is the concatenation, in key order, of the state keys whose name starts with "obs", flattened to F <=
512 components; component i becomes the byte clamp(rint((x_i - lo_i) * scale_i), 0, 127).  The trunk is
`envpool_amd.pgx.net.Net`'s, with H + 1 head rows: H = the number of actions of a Discrete space (a Gumbel-max sample of
softmax(logits)), or the dimension of a Box space (mu = logits, a fixed sigma per component, the clamped action goes to
the env and logp is the density of the raw one).  MultiDiscrete and Dict action spaces are refused (ValueError).

Legal-action masks and integer-vector actions are kind 2 (MASKED): one categorical over the legal actions, whose flat
index goes to the env as C <= 4 integer components.

    env = envpool.make("Minesweeper-v0", "gymnasium", num_envs=4096)
    actor = Actor.random(env, mask=True)      # obs:action_mask [10, 10]; the action is (row, col) = divmod(flat, 10)
    ro = env.rollout(horizon=32); ro.attach(actor, seed=1); ro.reset(); ro.collect()
    tr = actor.trainer(); tr.fit(ro, epochs=4, batch=4096)           # the loss runs over the legal actions only

A MEMORY actor (csrc/actor_memory.hip.h is the contract) is an ordinary one behind a gated recurrent cell in the same
integer arithmetic, for tasks whose observation does not hold the state: the cell turns the feature row and the env's
state h, M bytes, into the state h' the trunk reads.  The collector keeps h per env and zeroes it where episodes end.

    actor = Actor.random(env, hidden=64, memory=64)                  # MiniGrid's 7x7 view, a MuJoCo task without velocities
    ro.attach(actor, seed=1); ro.reset(); ro.collect()
    h0, h = ro.memory()                                              # the states slot 0 was evaluated with, and now
    m = actor.module(); out = m.unroll(obs, h0, mask)                # BPTT in torch; Actor.from_module(m) comes back
    m = m.to("cuda"); out = m.unroll(obs, h0, mask, kernels=True)    # BPTT in the training kernels"""
from __future__ import annotations

from typing import Any, Sequence

import numpy as np

from envpool_amd.pgx.net import MAX_INPUTS, Net

MAGIC = 0x41415045  # "EPAA"
VERSION = 1
HEADER_BYTES = 36
DISCRETE, BOX, MASKED = 0, 1, 2
MAX_COMPONENTS, MAX_ACTIONS = 4, 127
MEMORY_MAGIC = 0x4D415045  # "EPAM"
MEMORY_HEADER_BYTES = 24
MAX_SHIFT, MAX_BIAS = 24, 1 << 30


def _nvec(nvec: Any, actions: int) -> np.ndarray:
    """int32 [4]: the components' sizes padded with ones; their product must be H."""
    v = np.asarray([actions] if nvec is None else nvec, np.int64).reshape(-1)
    if not 1 <= len(v) <= MAX_COMPONENTS or (v < 1).any() or int(np.prod(v)) != actions:
        raise ValueError(f"actor: nvec = {v.tolist()} must be 1 .. {MAX_COMPONENTS} sizes of at least 1 whose product "
                         f"is H = {actions}")
    return np.concatenate([v, np.ones(MAX_COMPONENTS - len(v), np.int64)]).astype(np.int32)


def space_of(env_or_spec: Any, mask: Any = None) -> dict:
    """What an actor needs of an env, its spec or a dict with these entries: `features` F, `kind`, `actions` H, the
    Box bounds `low` / `high` (float32 [H], empty for a Discrete space) and the observation bounds `obs_low` /
    `obs_high` (float64 [F]); kind 2 (MASKED) adds `mask0` (the first mask component, or -1) and `nvec`.  `mask`: None
    (no mask), True (the one obs key whose name ends in "action_mask") or the key's name.  A Discrete space with a mask,
    and an integer Box (all lows 0, at most 4 components, at most 127 flat actions) with or without one, are MASKED.
    ValueError for F > 512, for an action space that is none of these, and for a mask that is missing, not of H
    components or asked for a float Box -- no device is needed."""
    if isinstance(env_or_spec, dict):
        d = dict(env_or_spec)
        if mask is not None:
            raise ValueError("actor: a dict states mask0 itself; mask= needs an env or a spec")
    else:
        spec = getattr(env_or_spec, "spec", env_or_spec)
        lows, highs, first = [], [], {}
        for key, s in spec.state_array_spec.items():
            if not key.startswith("obs"):
                continue
            n = int(np.prod([x for x in s.shape if x > 0], dtype=np.int64))  # (a spec writes a scalar per env as [-1])
            first[key] = (sum(len(x) for x in lows), n)
            lows.append(np.broadcast_to(np.asarray(s.minimum, np.float64).reshape(-1), (n,)) if np.size(s.minimum) in (1, n)
                        else np.full(n, -np.inf))
            highs.append(np.broadcast_to(np.asarray(s.maximum, np.float64).reshape(-1), (n,)) if np.size(s.maximum) in (1, n)
                         else np.full(n, np.inf))
        d = dict(obs_low=np.concatenate(lows), obs_high=np.concatenate(highs))
        d["features"] = len(d["obs_low"])
        space = spec.action_space
        name = type(space).__name__.lstrip("_")  # (gymnasium's classes, or the stand-ins used without it)
        if name == "Discrete":
            d.update(kind=DISCRETE, actions=int(space.n), low=np.zeros(0, np.float32), high=np.zeros(0, np.float32))
        elif name == "Box" and np.dtype(space.dtype).kind == "f":
            d.update(kind=BOX, actions=int(np.prod(space.shape, dtype=np.int64)),
                     low=np.asarray(space.low, np.float32).reshape(-1), high=np.asarray(space.high, np.float32).reshape(-1))
        elif name == "Box" and np.dtype(space.dtype).kind in "iu":
            high = np.asarray(space.high, np.int64).reshape(-1)
            if (np.asarray(space.low).reshape(-1) != 0).any() or not 1 <= len(high) <= MAX_COMPONENTS or (high < 0).any() \
                    or int(np.prod(high + 1)) > MAX_ACTIONS:
                raise ValueError(f"actor: an integer Box of low {space.low} and high {space.high} is not supported (all "
                                 f"lows 0, at most {MAX_COMPONENTS} components, at most {MAX_ACTIONS} flat actions)")
            d.update(kind=MASKED, actions=int(np.prod(high + 1)), mask0=-1, nvec=(high + 1).astype(np.int32),
                     low=np.zeros(0, np.float32), high=np.zeros(0, np.float32))
        else:
            raise ValueError(f"actor: an action space of {name} is not supported (Discrete or Box)")
        if mask is not None and mask is not False:
            names = [k for k in first if k.endswith("action_mask")] if mask is True else [mask]
            if len(names) != 1 or names[0] not in first:
                raise ValueError(f"actor: mask = {mask!r} names no obs key, or not exactly one (obs keys: {list(first)})")
            if d["kind"] == BOX:
                raise ValueError("actor: a float Box action space takes no mask")
            at, n = first[names[0]]
            if n != d["actions"]:
                raise ValueError(f"actor: the mask {names[0]!r} has {n} components for H = {d['actions']} actions")
            d.update(kind=MASKED, mask0=at, nvec=d.get("nvec", np.array([d["actions"]], np.int32)))
    if d["features"] > MAX_INPUTS:
        raise ValueError(f"actor: the observation has {d['features']} components; an actor takes at most {MAX_INPUTS}")
    if d["kind"] not in (DISCRETE, BOX, MASKED):
        raise ValueError(f"actor: kind = {d['kind']!r} must be 0 (discrete), 1 (box) or 2 (masked)")
    return d


class Actor:
    """`net`: the trunk and head, a `pgx.net.Net` of F inputs and H "actions"; `lo`, `scale`: float64 [F]; `sigma`,
    `low`, `high`: float32 [H] of a Box actor; `mask0`, `nvec`: the first mask component (-1: none) and the components'
    sizes of a MASKED actor.  `cell`: the two layers of a MEMORY actor's cell, ((Wz, bz, sz), (Wn, bn, sn)) with weights
    int8 [M, F + M] over [x ; h], biases int32 [M] and shifts 0 .. 24; the net then has M inputs, lo and scale are the
    F outer features', and `memory` is M (0 without a cell).  Everything the contract bounds is checked here
    (ValueError)."""

    def __init__(self, net: Net, kind: int, lo: Any, scale: Any, sigma: Any = None, low: Any = None, high: Any = None,
                 mask0: int = -1, nvec: Any = None, cell: Any = None):
        if kind not in (DISCRETE, BOX, MASKED):
            raise ValueError(f"actor: kind = {kind!r} must be 0 (discrete), 1 (box) or 2 (masked)")
        self.net, self.kind = net, int(kind)
        self.features, self.actions = net.inputs, net.actions
        self.memory, self.cell = 0, None
        if cell is not None:
            self.memory, self.features = net.inputs, int(np.size(lo))
            self.cell = self._check_cell(cell, self.features, self.memory)
            if self.kind == MASKED:
                raise ValueError("actor: a masked actor (kind 2) takes no memory: its mask indexes raw observation "
                                 "components")
        self.mask0, self.nvec = int(mask0), _nvec(nvec, net.actions)           # nvec: padded to 4 with ones
        self.components = 1 if nvec is None else int(np.size(np.asarray(nvec)))  # C: the entries given
        if self.kind != MASKED and (self.mask0 != -1 or self.components != 1):
            raise ValueError("actor: mask0 and nvec belong to a masked actor (kind 2)")
        if self.mask0 != -1 and not 0 <= self.mask0 <= self.features - self.actions:
            raise ValueError(f"actor: mask0 = {mask0} must be -1 or 0 .. F - H = {self.features - self.actions}")
        self.lo = np.ascontiguousarray(lo, np.float64).reshape(-1)
        self.scale = np.ascontiguousarray(scale, np.float64).reshape(-1)
        if self.lo.shape != (self.features,) or self.scale.shape != (self.features,):
            raise ValueError(f"actor: lo and scale must have {self.features} components")
        if not (np.isfinite(self.lo).all() and np.isfinite(self.scale).all()):
            raise ValueError("actor: lo and scale must be finite")
        box = self.kind == BOX
        h = self.actions if box else 0
        self.sigma = np.ascontiguousarray(sigma if box else np.zeros(0), np.float32).reshape(-1)
        self.low = np.ascontiguousarray(low if box else np.zeros(0), np.float32).reshape(-1)
        self.high = np.ascontiguousarray(high if box else np.zeros(0), np.float32).reshape(-1)
        if self.sigma.shape != (h,) or self.low.shape != (h,) or self.high.shape != (h,):
            raise ValueError(f"actor: sigma, low and high must have {h} components")
        if box and not (np.isfinite(self.sigma).all() and (self.sigma > 0).all()):
            raise ValueError("actor: sigma must be finite and above 0")
        if box and not (self.low <= self.high).all():
            raise ValueError("actor: low must not exceed high")

    @staticmethod
    def _check_cell(cell: Any, f: int, m: int) -> tuple:
        if m % 32 or not 32 <= m <= 512 or not 1 <= f <= MAX_INPUTS:
            raise ValueError(f"actor: memory = {m} must be a multiple of 32 in 32 .. 512 (F = {f} in 1 .. {MAX_INPUTS})")
        out = []
        for name, (w, b, shift) in zip(("Wz", "Wn"), cell):
            w, b, shift = np.asarray(w), np.asarray(b), int(shift)
            if w.shape != (m, f + m) or b.shape != (m,):
                raise ValueError(f"actor: cell layer {name}: weights {w.shape} and bias {b.shape} must be "
                                 f"({m}, {f + m}) and ({m},)")
            if np.any(w != np.rint(w)) or np.any(np.abs(w.astype(np.int64)) > 127):
                raise ValueError(f"actor: cell layer {name}: weights are -127 .. 127")
            if np.any(np.abs(b.astype(np.int64)) > MAX_BIAS) or not 0 <= shift <= MAX_SHIFT:
                raise ValueError(f"actor: cell layer {name}: |bias| <= 2^30 and shift 0 .. {MAX_SHIFT}")
            out.append((np.ascontiguousarray(w, np.int8), np.ascontiguousarray(b, np.int32), shift))
        return tuple(out)

    # -- the blob ------------------------------------------------------------------
    def blob(self) -> np.ndarray:
        """The actor as the C ABI takes it (include/envpool_amd.h: epa_actor_begin): uint8, 4-byte aligned.  A memory
        actor: the EPAM wrapper around the inner actor's EPAA blob (F = M, lo 0, scale 1)."""
        n = self.net
        if self.memory:
            parts = [np.array([MEMORY_MAGIC, VERSION, self.features, self.memory, 0, 0], "<u4").tobytes(),
                     self.lo.astype("<f8").tobytes(), self.scale.astype("<f8").tobytes()]
            for w, b, shift in self.cell:
                raw = w.tobytes()
                parts += [raw, b"\0" * (-len(raw) % 4), b.astype("<i4").tobytes(), np.array([shift], "<i4").tobytes()]
            inner = Actor(n, self.kind, np.zeros(self.memory), np.ones(self.memory), self.sigma, self.low, self.high)
            parts.append(inner.blob().tobytes())
            return np.frombuffer(b"".join(parts), np.uint8).copy()
        parts = [np.array([MAGIC, VERSION, self.features, self.actions, n.hidden, n.blocks, self.kind], "<u4").tobytes(),
                 np.array([n.scale_p, n.scale_v], "<f4").tobytes(), self.lo.astype("<f8").tobytes(),
                 self.scale.astype("<f8").tobytes()]
        if self.kind == BOX:
            parts.append(self.sigma.astype("<f4").tobytes())
        if self.kind == MASKED:
            parts.append(np.array([self.mask0, self.components, *self.nvec], "<i4").tobytes())
        parts.append(n.blob()[32:].tobytes())  # the layer section, exactly as Net writes it
        return np.frombuffer(b"".join(parts), np.uint8).copy()

    def save(self, path: str) -> None:
        n = self.net
        arrays = {"kind": np.int32(self.kind), "features": np.int32(self.features), "actions": np.int32(self.actions),
                  "hidden": np.int32(n.hidden), "blocks": np.int32(n.blocks),
                  "net_scale": np.array([n.scale_p, n.scale_v], np.float32),
                  "shift": np.array([s for _, _, s in n.layers], np.int32), "lo": self.lo, "scale": self.scale,
                  "sigma": self.sigma, "low": self.low, "high": self.high, "mask0": np.int32(self.mask0),
                  "nvec": self.nvec[:self.components], "memory": np.int32(self.memory)}
        for i, (w, b, _) in enumerate(n.layers):
            arrays[f"w{i}"], arrays[f"b{i}"] = w, b
        for name, (w, b, shift) in zip("zn", self.cell or ()):
            arrays[f"cell_w{name}"], arrays[f"cell_b{name}"], arrays[f"cell_s{name}"] = w, b, np.int32(shift)
        with open(path, "wb") as f:  # (np.savez would add ".npz" to a bare name)
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path: str) -> "Actor":
        with np.load(path) as z:
            blocks = int(z["blocks"])
            layers = [(z[f"w{i}"], z[f"b{i}"], int(z["shift"][i])) for i in range(2 * blocks + 2)]
            memory = int(z["memory"]) if "memory" in z.files else 0
            net = Net((memory or int(z["features"]),), int(z["actions"]), int(z["hidden"]), blocks, layers,
                      float(z["net_scale"][0]), float(z["net_scale"][1]))
            masked = dict(mask0=int(z["mask0"]), nvec=z["nvec"]) if int(z["kind"]) == MASKED else {}
            cell = tuple((z[f"cell_w{g}"], z[f"cell_b{g}"], int(z[f"cell_s{g}"])) for g in "zn") if memory else None
            return cls(net, int(z["kind"]), z["lo"], z["scale"], z["sigma"], z["low"], z["high"], cell=cell, **masked)

    @classmethod
    def random(cls, env_or_spec: Any, hidden: int = 64, blocks: int = 1, seed: int = 0, sigma: float = 0.5,
               mask: Any = None, memory: int = 0) -> "Actor":
        """An actor for tests and first runs from numpy's PCG64(seed) (`Net.random`'s recipe, shifts for inputs that
        fill 0 .. 127).  lo / scale map an observation component's bounds onto 0 .. 127 where the spec gives finite
        ones no wider than 1e6, and -8 .. 8 elsewhere; `fit_features` replaces them by measured ones.  `mask`: as
        `space_of`'s.  `memory` = M: a memory actor, whose trunk has M inputs behind a random cell (PCG64(seed + 1);
        shifts that spread the gate and the candidate over their ranges)."""
        d = space_of(env_or_spec, mask)
        f, h = int(d["features"]), int(d["actions"])
        if isinstance(memory, (bool, np.bool_)) or not isinstance(memory, (int, np.integer)) or memory < 0:
            raise ValueError(f"actor: memory = {memory!r} must be an integer of at least 0")
        f_net, cell = int(memory) or f, None
        if memory:
            rng = np.random.Generator(np.random.PCG64(seed + 1))
            shift = min(MAX_SHIFT, int(round(np.log2(73.0 * np.sqrt(f + memory) * 74.0 / 40.0))))
            cell = tuple((rng.integers(-127, 128, size=(memory, f + memory)).astype(np.int8),
                          rng.integers(-1024, 1025, size=memory).astype(np.int32), shift) for _ in range(2))
        # (Net.random sizes the first shift for 0 / 1 inputs of density 1/4; bytes spread over 0 .. 127 are about
        # 2^7 larger)
        net = Net.random((f_net,), h, hidden, blocks, seed)
        w, b, s = net.layers[0]
        net = Net((f_net,), h, hidden, blocks, [(w, b, min(24, s + 7))] + net.layers[1:], net.scale_p, net.scale_v)
        lo, hi = np.asarray(d["obs_low"], np.float64), np.asarray(d["obs_high"], np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            span = hi - lo
        ok = np.isfinite(lo) & np.isfinite(hi) & (span > 0) & (span <= 1e6)
        lo = np.where(ok, lo, -8.0)
        scale = 127.0 / np.where(ok, span, 16.0)
        masked = dict(mask0=d.get("mask0", -1), nvec=d.get("nvec")) if d["kind"] == MASKED else {}
        return cls(net, d["kind"], lo, scale, np.full(h, sigma, np.float32), d["low"], d["high"], cell=cell, **masked)

    def fit_features(self, cnt: Any, s1: Any, s2: Any) -> "Actor":
        """lo and scale from a collector's moments (`ro.moments()`): mean +- 4 sigma of every component onto 0 .. 127.
        The moments cover the float obs keys, so they must have F components; a component without spread keeps its
        lo and scale."""
        cnt, s1, s2 = (np.asarray(x, np.float64).reshape(-1) for x in (cnt, s1, s2))
        if not cnt.shape == s1.shape == s2.shape == (self.features,):
            raise ValueError(f"actor: moments of {cnt.shape[0]} components for {self.features} features")
        mean = s1 / cnt
        std = np.sqrt(np.maximum(s2 / cnt - mean * mean, 0.0))
        ok = np.isfinite(mean) & np.isfinite(std) & (std > 0)
        self.lo = np.where(ok, mean - 4.0 * std, self.lo)
        self.scale = np.where(ok, 127.0 / np.where(ok, 8.0 * std, 1.0), self.scale)
        return self

    def features_of(self, obs: Sequence[Any]) -> np.ndarray:
        """The feature bytes uint8 [rows, F] of observation arrays, one per obs key in key order (numpy, the contract's
        arithmetic)."""
        x = np.concatenate([np.asarray(o).reshape(len(o), -1).astype(np.float64) for o in obs], axis=1)
        with np.errstate(invalid="ignore", over="ignore"):
            p = (x - self.lo) * self.scale
        r = np.clip(np.rint(np.where(np.isfinite(p), p, 0.0)), 0, 127)
        return r.astype(np.uint8)

    # -- the torch twin ------------------------------------------------------------
    def module(self, kernels: bool = False) -> Any:
        """A `torch.nn.Module` with this actor's numbers: `features(obs)` the contract's bytes as float64 (rounding
        passes gradients straight through), `integers(obs)` the head's p as float64 -- exactly the device's --,
        `forward(obs) -> (logits float32 [rows, H], value float32 [rows])` with the contract's bits, and the
        differentiable `logp(obs, action)`, `entropy(obs)` and `value(obs)` a learner needs.  `obs`: a tensor [rows, ...]
        (several obs keys: concatenated along the flattened last axis in key order).  The trunk is `Net.module()`'s;
        sigma is a parameter.  `kernels` goes to the trunk (`Net.module(kernels=True)`: the training kernels for obs on
        a ROCm device); the features stay torch, and obs must not require grad.  `logp_of(logits, action)` is `logp`
        from the logits of one `forward(obs)`, which then serves the value too: one pass through the trunk per step.
        A MEMORY actor's module adds `cell(features, h) -> h'` (float64, the contract's integers, rounding passes
        gradients straight through) and `unroll(obs [T, N, ...], h0 [N, M], mask [T, N]) -> (logits [T, N, H], value
        [T, N], h [N, M])` under the state rule, for BPTT in torch; `integers`, `forward`, `logp`, `entropy` and
        `value` take the state as `h=` (default: zeros).  `module(kernels=True)` is a ValueError for it: its training
        kernels are a per-call switch, `unroll(obs, h0, mask, kernels=True)` (actor_memory_train.py)."""
        if self.memory and kernels:
            raise ValueError("actor: module(kernels=True) is not available for a memory actor: the training kernels "
                             "have no cell; train by BPTT with module()")
        return _make_module(self, bool(kernels))

    def trainer(self, **options: Any) -> Any:
        """An `ActorTrainer` of this actor (actor_trainer.py): PPO on the device.  `device=0, optimizer="adam", lr=3e-2,
        betas=(0.9, 0.999), eps=1e-8, momentum=0.9, weight_decay=0.0, clip_ratio=0.2, value_weight=0.5,
        entropy_weight=0.0, normalize_adv=True, train_sigma=True, clip=0.5, seed=0, max_rows=4096`."""
        from envpool_amd.actor_trainer import ActorTrainer

        if self.memory:
            raise ValueError("actor: trainer() is not available for a memory actor: the PPO trainer's kernels have no "
                             "backward pass through time; train by BPTT with module()")
        return ActorTrainer(self, **options)

    @classmethod
    def from_module(cls, m: Any) -> "Actor":
        sigma = m.sigma.detach().cpu().numpy().astype(np.float32) if m.kind == BOX else None
        masked = dict(mask0=m.mask0, nvec=m.nvec) if m.kind == MASKED else {}
        cell = None
        if m.memory:
            cell = tuple((np.clip(np.rint(w.detach().cpu().numpy()), -127, 127).astype(np.int8),
                          np.clip(np.rint(b.detach().cpu().numpy()), -MAX_BIAS, MAX_BIAS).astype(np.int32), int(s))
                         for w, b, s in zip(m.cell_weights, m.cell_biases, m.cell_shifts))
        return cls(Net.from_module(m.net), m.kind, m.lo.cpu().numpy(), m.scale.cpu().numpy(), sigma, m.low, m.high,
                   cell=cell, **masked)


def _make_module(actor: Actor, kernels: bool = False) -> Any:
    import torch

    class ActorModule(torch.nn.Module):
        def __init__(self) -> None:
            super().__init__()
            self.kind, self.actions = actor.kind, actor.actions
            self.low, self.high = actor.low.copy(), actor.high.copy()
            self.mask0, self.nvec = actor.mask0, actor.nvec[:actor.components].copy()
            self.net = actor.net.module(kernels=kernels)
            self.register_buffer("lo", torch.tensor(actor.lo))
            self.register_buffer("scale", torch.tensor(actor.scale))
            self.sigma = torch.nn.Parameter(torch.tensor(actor.sigma.astype(np.float32)))
            self.memory = actor.memory
            if actor.memory:
                self.cell_shifts = [s for _, _, s in actor.cell]
                self.cell_weights = torch.nn.ParameterList(
                    [torch.nn.Parameter(torch.tensor(w.astype(np.float64))) for w, _, _ in actor.cell])
                self.cell_biases = torch.nn.ParameterList(
                    [torch.nn.Parameter(torch.tensor(b.astype(np.float64))) for _, b, _ in actor.cell])

        def _cell_layer(self, i: int, v: Any) -> Any:
            ste = self.net._ste
            w = ste(self.cell_weights[i], torch.clamp(torch.round(self.cell_weights[i]), -127, 127))
            b = ste(self.cell_biases[i], torch.round(self.cell_biases[i]))
            z, s = v @ w.t() + b, self.cell_shifts[i]
            return ste(z / 2.0 ** s, torch.floor((z + 2.0 ** (s - 1)) / 2.0 ** s)) if s else z

        def cell(self, features: Any, h: Any) -> Any:
            """h' float64 [rows, M] of the feature rows [rows, F] and the states h [rows, M]: the contract's integers."""
            h = h.to(torch.float64)
            v = torch.cat([features.to(torch.float64), h], dim=1)
            z = torch.clamp(64.0 + self._cell_layer(0, v), 0, 128)
            n = torch.clamp(self._cell_layer(1, v), 0, 127)
            y = (z * h + (128.0 - z) * n + 64.0) / 128.0
            return self.net._ste(y, torch.floor(y))

        def unroll(self, obs: Any, h0: Any, mask: Any, kernels: bool = False) -> tuple[Any, Any, Any]:
            """(logits float32 [T, N, H], value float32 [T, N], h float64 [N, M]) of obs [T, N, ...] from the states h0
            under the state rule: slot t is evaluated with the state as it is, and the state is zero after a slot
            whose mask[t, n] is False.  `kernels=True`: for obs on a ROCm device the cell's unroll, the trunk and the
            backward through time are the training kernels (csrc/actor_memory_train.hip.h: the same integers, every
            gradient within 2.6e-4 per step of depth of this code's); the features stay torch, obs must not require
            grad, T N is at most 2^20 and the parameters, h0 and mask are on obs's device (ValueError).  On CPU
            tensors it is this code."""
            if kernels:
                from envpool_amd import actor_memory_train

                if obs.requires_grad:
                    raise ValueError("actor: kernels=True computes no gradient for the observation; obs must not "
                                     "require grad")
                if self.cell_weights[0].device != obs.device:
                    raise ValueError(f"actor: the parameters are on {self.cell_weights[0].device} and obs on "
                                     f"{obs.device}; move the module to obs's device")
                if obs.is_cuda:
                    t, n = int(obs.shape[0]), int(obs.shape[1])
                    x8 = torch.round(self.features(obs.reshape((t * n,) + tuple(obs.shape[2:]))))
                    x8 = x8.to(torch.uint8).reshape(t, n, -1)
                    p, h = actor_memory_train.unroll_integers(self, x8, h0, mask)
                    p = p.to(torch.float32).reshape(t, n, -1)
                    return (p[:, :, :self.actions] * torch.tensor(self.net.scale_p, dtype=torch.float32),
                            p[:, :, self.actions] * torch.tensor(self.net.scale_v, dtype=torch.float32), h)
            h, logits, values = h0.to(torch.float64), [], []
            for t in range(obs.shape[0]):
                h = self.cell(self.features(obs[t]), h)
                p = self.net.integers(h).to(torch.float32)
                logits.append(p[:, :self.actions] * torch.tensor(self.net.scale_p, dtype=torch.float32))
                values.append(p[:, self.actions] * torch.tensor(self.net.scale_v, dtype=torch.float32))
                h = h * mask[t].to(torch.float64).reshape(-1, 1)
            return torch.stack(logits), torch.stack(values), h

        def features(self, obs: Any) -> Any:
            x = obs.reshape(obs.shape[0], -1).to(torch.float64)
            p = (x - self.lo) * self.scale
            p = torch.where(torch.isfinite(p), p, torch.zeros_like(p))
            return p + (torch.clamp(torch.round(p), 0, 127) - p).detach()  # (torch.round: half to even)

        def integers(self, obs: Any, h: Any = None) -> Any:
            x = self.features(obs)
            if self.memory:
                zeros = torch.zeros((x.shape[0], self.memory), dtype=torch.float64, device=x.device)
                x = self.cell(x, zeros if h is None else h)
            return self.net.integers(x)

        def forward(self, obs: Any, h: Any = None) -> tuple[Any, Any]:
            p = self.integers(obs, h).to(torch.float32)
            logits = p[:, :self.actions] * torch.tensor(self.net.scale_p, dtype=torch.float32)
            value = p[:, self.actions] * torch.tensor(self.net.scale_v, dtype=torch.float32)
            return logits, value

        def value(self, obs: Any, h: Any = None) -> Any:
            return self.forward(obs, h)[1]

        def legal(self, obs: Any) -> Any:
            """bool [rows, H] of a MASKED actor: the raw mask components of `obs` that are not 0; every action for a row
            without any, and for an actor without a mask."""
            rows = obs.shape[0]
            if self.mask0 < 0:
                return torch.ones((rows, self.actions), dtype=torch.bool, device=obs.device)
            ok = obs.reshape(rows, -1)[:, self.mask0:self.mask0 + self.actions] != 0
            return ok | ~ok.any(dim=1, keepdim=True)

        def _masked(self, logits: Any, legal: Any) -> Any:
            """log-softmax over the legal actions, float64; -inf at the others."""
            return torch.log_softmax(logits.to(torch.float64).masked_fill(~legal, -torch.inf), dim=1)

        def logp(self, obs: Any, action: Any, h: Any = None) -> Any:
            """float64 [rows]: the log-probability (Box: the density) of `action` from the float32 logits.  MASKED:
            `action` is the flat index, or its [rows, C] components."""
            return self.logp_of(self.forward(obs, h)[0], action, self.legal(obs) if self.kind == MASKED else None)

        def logp_of(self, logits: Any, action: Any, legal: Any = None) -> Any:
            """`logp` from the logits of a `forward(obs)` the caller already has: one pass serves `logp` and value.
            MASKED: `legal` is `self.legal(obs)` (None: every action)."""
            if self.kind == MASKED:
                if action.dim() == 2:  # components, most significant first
                    flat = torch.zeros_like(action[:, 0])
                    for c, n in enumerate(self.nvec):
                        flat = flat * int(n) + action[:, c]
                    action = flat
                legal = torch.ones_like(logits, dtype=torch.bool) if legal is None else legal
                return self._masked(logits, legal).gather(1, action.reshape(-1, 1).long()).reshape(-1)
            logits = logits.to(torch.float64)
            if self.kind == DISCRETE:
                return torch.log_softmax(logits, dim=1).gather(1, action.reshape(-1, 1).long()).reshape(-1)
            sigma = self.sigma.to(torch.float64)
            z = (action.reshape(logits.shape).to(torch.float64) - logits) / sigma
            return (-0.5 * z * z - torch.log(sigma) - 0.9189385).sum(dim=1)

        def entropy(self, obs: Any, h: Any = None) -> Any:
            logits = self.forward(obs, h)[0].to(torch.float64)
            if self.kind == MASKED:
                legal = self.legal(obs)
                lp = self._masked(logits, legal).masked_fill(~legal, 0.0)  # (no -inf reaches a product)
                return -(lp.exp() * lp * legal).sum(dim=1)
            if self.kind == DISCRETE:
                lp = torch.log_softmax(logits, dim=1)
                return -(lp.exp() * lp).sum(dim=1)
            return (0.5 + 0.9189385 + torch.log(self.sigma.to(torch.float64))).sum().expand(logits.shape[0])

    return ActorModule()
