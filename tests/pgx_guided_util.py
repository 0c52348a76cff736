"""The PGX guided tree search (envpool_amd/csrc/pgx_guided.hip.h, DESIGN.md "PGX guided search") restated in Python
and numpy, independently of the header: the tree of one root is kept here, positions and expansion steps come from the
caller (the reference-pinned replay on the CPU, public pool calls on the GPU), scores are computed in np.float32
operation by operation.  And a deterministic stand-in evaluator: float32 priors and a float32 value from an integer
hash of the bytes of `obs` and `mask`, no RNG."""
from typing import Any, Callable, NamedTuple

import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max


class Pos(NamedTuple):
    """A position as the guided search sees it."""

    mask: np.ndarray  # bool [A]: info:legal_action_mask
    done: bool
    mover: int        # info:current_player
    obs: np.ndarray   # bool [H, W, C]: the mover's obs row
    key: Any          # whatever the caller's expand needs to find the position again


def clean(x):
    x = F(x)
    return x if (x >= 0 and x <= FLT_MAX) else F(0.0)


def cleanv(x):
    x = F(x)
    return x if (x >= -1 and x <= 1) else F(0.0)


def score(v, w0, p, total, sign, c_puct):
    """score(node, a) of the contract; every operation rounds to float32."""
    q = (F(sign) * F(w0)) / F(int(v)) if v > 0 else F(0.0)
    u = (F(c_puct) * F(p)) * np.sqrt(F(int(total) + 1))
    out = q + u / F(1 + int(v))
    assert isinstance(out, np.float32)
    return out


class GuidedTree:
    """One root's session: begin is the constructor, then `leaf()`, `advance(priors_row, value)`, `result()`.
    expand(pos, a) -> (the position after a, seat 0's reward of that step)."""

    def __init__(self, root: Pos, over: bool, expand: Callable[[Pos, int], tuple], simulations: int, c_puct: float):
        self.n_act = len(root.mask)
        self.expand, self.S, self.c = expand, simulations, c_puct
        self.nodes = []
        self.over = over
        self._make(root, 0)
        self.path, self.pending, self.status, self.t = [], 0, 2 if over else 0, 0

    def _make(self, pos, term0):
        n = self.n_act
        self.nodes.append(dict(pos=pos, term0=term0, child=[-1] * n, v=[0] * n, w0=[F(0.0)] * n, p=[F(0.0)] * n))
        return len(self.nodes) - 1

    def leaf(self):
        """(obs, mask, status) of the pending leaf: zeros unless status 0."""
        pos = self.nodes[self.pending]["pos"]
        if self.status != 0:
            return np.zeros_like(self.nodes[0]["pos"].obs), np.zeros(self.n_act, bool), self.status
        return pos.obs, pos.mask, 0

    def advance(self, priors, value):
        assert self.t <= self.S
        t, self.t = self.t, self.t + 1
        if self.status == 2:
            return
        leaf = self.nodes[self.pending]
        if self.status == 0:
            leaf["p"] = [clean(x) for x in priors]
            val0 = F(1 if leaf["pos"].mover == 0 else -1) * cleanv(value)
        else:
            val0 = F(leaf["term0"])
        for n, a in self.path:
            self.nodes[n]["v"][a] += 1
            self.nodes[n]["w0"][a] = F(self.nodes[n]["w0"][a] + val0)
        if t == self.S:
            self.status = 2
            return
        node, self.path = 0, []
        while True:
            nd = self.nodes[node]
            total = sum(nd["v"])
            sign = 1 if nd["pos"].mover == 0 else -1
            best, a = None, -1
            for b in np.flatnonzero(nd["pos"].mask):
                s = score(nd["v"][b], nd["w0"][b], nd["p"][b], total, sign, self.c)
                if best is None or s > best:
                    best, a = s, int(b)
            assert a >= 0
            self.path.append((node, a))
            if nd["child"][a] < 0:
                pos, term0 = self.expand(nd["pos"], a)
                node = nd["child"][a] = self._make(pos, term0)
                break
            node = nd["child"][a]
            if self.nodes[node]["pos"].done:
                break
        self.pending = node
        self.status = 1 if self.nodes[node]["pos"].done else 0
        assert len(self.nodes) <= self.S + 1

    def result(self):
        """(visits int32 [A], values float32 [A], action, nodes)"""
        root = self.nodes[0]
        if self.over:
            return np.zeros(self.n_act, np.int32), np.zeros(self.n_act, F), -1, len(self.nodes)
        visits = np.array(root["v"], np.int32)
        sign = F(1 if root["pos"].mover == 0 else -1)
        values = np.array([sign * F(w) for w in root["w0"]], F)
        legal = np.flatnonzero(root["pos"].mask)
        return visits, values, int(legal[np.argmax(visits[legal])]), len(self.nodes)


def stand_in(obs, mask):
    """The stand-in evaluator: (priors float32 [k, A], values float32 [k]) from the bytes of obs [k, ...] and
    mask [k, A].  An integer hash per row, a second one per action; priors are the legal actions' hashes over their
    integer sum, divided in float32; the value is 24 hash bits mapped to [-1, 1).  Rows of zeros get zeros priors."""
    obs = np.ascontiguousarray(obs).view(np.uint8).reshape(len(obs), -1).astype(np.uint64)
    mask = np.ascontiguousarray(mask).view(np.uint8).reshape(len(mask), -1).astype(np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    both = np.concatenate([obs, mask], axis=1)
    w = (np.arange(both.shape[1], dtype=np.uint64) * np.uint64(2654435761) + np.uint64(40503)) & m32
    h = ((both * w[None, :]).sum(1) + np.uint64(0x9E3779B9)) & m32
    h = ((h ^ (h >> np.uint64(15))) * np.uint64(0x85EBCA6B)) & m32
    act = np.arange(mask.shape[1], dtype=np.uint64)
    x = ((h[:, None] ^ ((act[None, :] + np.uint64(1)) * np.uint64(0x9E3779B1) & m32)) * np.uint64(0xC2B2AE35)) & m32
    x = ((x >> np.uint64(12)) + np.uint64(1)) * mask  # 1 .. 2^20 on legal actions
    total = x.sum(1)
    priors = x.astype(F) / np.maximum(total, np.uint64(1)).astype(F)[:, None]
    values = ((h >> np.uint64(8)).astype(F) / F(2.0**23) - F(1.0)).astype(F)
    assert priors.dtype == F and values.dtype == F
    return np.ascontiguousarray(priors), np.ascontiguousarray(values)
