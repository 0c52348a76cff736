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
the env and logp is the density of the raw one).  MultiDiscrete and Dict action spaces are refused (ValueError)."""
from __future__ import annotations

from typing import Any, Sequence

import numpy as np

from envpool_amd.pgx.net import MAX_INPUTS, Net

MAGIC = 0x41415045  # "EPAA"
VERSION = 1
HEADER_BYTES = 36
DISCRETE, BOX = 0, 1


def space_of(env_or_spec: Any) -> dict:
    """What an actor needs of an env, its spec or a dict with these entries: `features` F, `kind`, `actions` H, the
    Box bounds `low` / `high` (float32 [H], empty for a Discrete space) and the observation bounds `obs_low` /
    `obs_high` (float64 [F]).  ValueError for F > 512 and for an action space that is neither Discrete nor Box -- no
    device is needed."""
    if isinstance(env_or_spec, dict):
        d = dict(env_or_spec)
    else:
        spec = getattr(env_or_spec, "spec", env_or_spec)
        lows, highs = [], []
        for key, s in spec.state_array_spec.items():
            if not key.startswith("obs"):
                continue
            n = int(np.prod([x for x in s.shape if x > 0], dtype=np.int64))  # (a spec writes a scalar per env as [-1])
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
        else:
            raise ValueError(f"actor: an action space of {name} is not supported (Discrete or Box)")
    if d["features"] > MAX_INPUTS:
        raise ValueError(f"actor: the observation has {d['features']} components; an actor takes at most {MAX_INPUTS}")
    if d["kind"] not in (DISCRETE, BOX):
        raise ValueError(f"actor: kind = {d['kind']!r} must be 0 (discrete) or 1 (box)")
    return d


class Actor:
    """`net`: the trunk and head, a `pgx.net.Net` of F inputs and H "actions"; `lo`, `scale`: float64 [F]; `sigma`,
    `low`, `high`: float32 [H] of a Box actor.  Everything the contract bounds is checked here (ValueError)."""

    def __init__(self, net: Net, kind: int, lo: Any, scale: Any, sigma: Any = None, low: Any = None, high: Any = None):
        if kind not in (DISCRETE, BOX):
            raise ValueError(f"actor: kind = {kind!r} must be 0 (discrete) or 1 (box)")
        self.net, self.kind = net, int(kind)
        self.features, self.actions = net.inputs, net.actions
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

    # -- the blob ------------------------------------------------------------------
    def blob(self) -> np.ndarray:
        """The actor as the C ABI takes it (include/envpool_amd.h: epa_actor_begin): uint8, 4-byte aligned."""
        n = self.net
        parts = [np.array([MAGIC, VERSION, self.features, self.actions, n.hidden, n.blocks, self.kind], "<u4").tobytes(),
                 np.array([n.scale_p, n.scale_v], "<f4").tobytes(), self.lo.astype("<f8").tobytes(),
                 self.scale.astype("<f8").tobytes()]
        if self.kind == BOX:
            parts.append(self.sigma.astype("<f4").tobytes())
        parts.append(n.blob()[32:].tobytes())  # the layer section, exactly as Net writes it
        return np.frombuffer(b"".join(parts), np.uint8).copy()

    def save(self, path: str) -> None:
        n = self.net
        arrays = {"kind": np.int32(self.kind), "features": np.int32(self.features), "actions": np.int32(self.actions),
                  "hidden": np.int32(n.hidden), "blocks": np.int32(n.blocks),
                  "net_scale": np.array([n.scale_p, n.scale_v], np.float32),
                  "shift": np.array([s for _, _, s in n.layers], np.int32), "lo": self.lo, "scale": self.scale,
                  "sigma": self.sigma, "low": self.low, "high": self.high}
        for i, (w, b, _) in enumerate(n.layers):
            arrays[f"w{i}"], arrays[f"b{i}"] = w, b
        with open(path, "wb") as f:  # (np.savez would add ".npz" to a bare name)
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path: str) -> "Actor":
        with np.load(path) as z:
            blocks = int(z["blocks"])
            layers = [(z[f"w{i}"], z[f"b{i}"], int(z["shift"][i])) for i in range(2 * blocks + 2)]
            net = Net((int(z["features"]),), int(z["actions"]), int(z["hidden"]), blocks, layers,
                      float(z["net_scale"][0]), float(z["net_scale"][1]))
            return cls(net, int(z["kind"]), z["lo"], z["scale"], z["sigma"], z["low"], z["high"])

    @classmethod
    def random(cls, env_or_spec: Any, hidden: int = 64, blocks: int = 1, seed: int = 0, sigma: float = 0.5) -> "Actor":
        """An actor for tests and first runs from numpy's PCG64(seed) (`Net.random`'s recipe, shifts for inputs that
        fill 0 .. 127).  lo / scale map an observation component's bounds onto 0 .. 127 where the spec gives finite
        ones no wider than 1e6, and -8 .. 8 elsewhere; `fit_features` replaces them by measured ones."""
        d = space_of(env_or_spec)
        f, h = int(d["features"]), int(d["actions"])
        # (Net.random sizes the first shift for 0 / 1 inputs of density 1/4; bytes spread over 0 .. 127 are about
        # 2^7 larger)
        net = Net.random((f,), h, hidden, blocks, seed)
        w, b, s = net.layers[0]
        net = Net((f,), h, hidden, blocks, [(w, b, min(24, s + 7))] + net.layers[1:], net.scale_p, net.scale_v)
        lo, hi = np.asarray(d["obs_low"], np.float64), np.asarray(d["obs_high"], np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            span = hi - lo
        ok = np.isfinite(lo) & np.isfinite(hi) & (span > 0) & (span <= 1e6)
        lo = np.where(ok, lo, -8.0)
        scale = 127.0 / np.where(ok, span, 16.0)
        return cls(net, d["kind"], lo, scale, np.full(h, sigma, np.float32), d["low"], d["high"])

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
    def module(self) -> Any:
        """A `torch.nn.Module` with this actor's numbers: `features(obs)` the contract's bytes as float64 (rounding
        passes gradients straight through), `integers(obs)` the head's p as float64 -- exactly the device's --,
        `forward(obs) -> (logits float32 [rows, H], value float32 [rows])` with the contract's bits, and the
        differentiable `logp(obs, action)`, `entropy(obs)` and `value(obs)` a learner needs.  `obs`: a tensor [rows, ...]
        (several obs keys: concatenated along the flattened last axis in key order).  The trunk is `Net.module()`'s;
        sigma is a parameter."""
        return _make_module(self)

    @classmethod
    def from_module(cls, m: Any) -> "Actor":
        sigma = m.sigma.detach().cpu().numpy().astype(np.float32) if m.kind == BOX else None
        return cls(Net.from_module(m.net), m.kind, m.lo.cpu().numpy(), m.scale.cpu().numpy(), sigma, m.low, m.high)


def _make_module(actor: Actor) -> Any:
    import torch

    class ActorModule(torch.nn.Module):
        def __init__(self) -> None:
            super().__init__()
            self.kind, self.actions = actor.kind, actor.actions
            self.low, self.high = actor.low.copy(), actor.high.copy()
            self.net = actor.net.module()
            self.register_buffer("lo", torch.tensor(actor.lo))
            self.register_buffer("scale", torch.tensor(actor.scale))
            self.sigma = torch.nn.Parameter(torch.tensor(actor.sigma.astype(np.float32)))

        def features(self, obs: Any) -> Any:
            x = obs.reshape(obs.shape[0], -1).to(torch.float64)
            p = (x - self.lo) * self.scale
            p = torch.where(torch.isfinite(p), p, torch.zeros_like(p))
            return p + (torch.clamp(torch.round(p), 0, 127) - p).detach()  # (torch.round: half to even)

        def integers(self, obs: Any) -> Any:
            return self.net.integers(self.features(obs))

        def forward(self, obs: Any) -> tuple[Any, Any]:
            p = self.integers(obs).to(torch.float32)
            logits = p[:, :self.actions] * torch.tensor(self.net.scale_p, dtype=torch.float32)
            value = p[:, self.actions] * torch.tensor(self.net.scale_v, dtype=torch.float32)
            return logits, value

        def value(self, obs: Any) -> Any:
            return self.forward(obs)[1]

        def logp(self, obs: Any, action: Any) -> Any:
            """float64 [rows]: the log-probability (Box: the density) of `action` from the float32 logits."""
            logits = self.forward(obs)[0].to(torch.float64)
            if self.kind == DISCRETE:
                return torch.log_softmax(logits, dim=1).gather(1, action.reshape(-1, 1).long()).reshape(-1)
            sigma = self.sigma.to(torch.float64)
            z = (action.reshape(logits.shape).to(torch.float64) - logits) / sigma
            return (-0.5 * z * z - torch.log(sigma) - 0.9189385).sum(dim=1)

        def entropy(self, obs: Any) -> Any:
            logits = self.forward(obs)[0].to(torch.float64)
            if self.kind == DISCRETE:
                lp = torch.log_softmax(logits, dim=1)
                return -(lp.exp() * lp).sum(dim=1)
            return (0.5 + 0.9189385 + torch.log(self.sigma.to(torch.float64))).sum().expand(logits.shape[0])

    return ActorModule()
