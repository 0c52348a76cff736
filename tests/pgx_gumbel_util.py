"""The PGX Gumbel search (envpool_amd/csrc/pgx_gumbel.hip.h, DESIGN.md "PGX Gumbel search") restated in Python and
numpy float32, independently of the header: the tree of one root is kept here, positions and expansion steps come from
the caller (the reference-pinned replay on the CPU), every float operation rounds to float32 in the contract's order,
the exponential and the wave's order of summation are restated, and the table of considered visits is the SEQUENCE form
of sequential halving (the header walks it in integers instead).  And deterministic stand-in evaluators that return
logits."""
from typing import Callable

import numpy as np

from pgx_guided_util import Pos, cleanv, stand_in

F = np.float32
FLT_MAX = np.finfo(np.float32).max
FLT_MIN = np.finfo(np.float32).tiny
BIG = F(1e30)
_LANES = np.arange(64)


def exp_(x):
    """The contract's exponential on float32 (scalar or array): the argument clamped to [-87, 0]."""
    x = np.asarray(x, F)
    x = np.minimum(np.maximum(x, F(-87.0)), F(0.0))
    k = np.rint(x * F(1.44269504))
    r = (x - k * F(0.693359375)) - k * F(-2.12194440e-4)
    p = F(1.0) / F(720.0)
    for c in (F(1.0) / F(120.0), F(1.0) / F(24.0), F(1.0) / F(6.0), F(0.5), F(1.0), F(1.0)):
        p = p * r + c
    out = np.ldexp(p, k.astype(np.int32))
    assert out.dtype == F
    return out


def wave_sum(terms):
    """A float32 sum over actions in the wave's order: terms[a] is +0.0 where a takes no part; lane j's partial is
    terms[j] + terms[j + 64], then the butterfly over lane distances 32 .. 1."""
    t = np.zeros(128, F)
    t[:len(terms)] = terms
    x = t[:64] + t[64:]
    for w in (32, 16, 8, 4, 2, 1):
        x = x + x[_LANES ^ w]
    assert x.dtype == F and len(np.unique(x.view(np.uint32))) == 1  # every lane holds the same bits
    return x[0]


def sequence_of_considered_visits(m, simulations):
    """Sequential halving as a sequence: entry t is the visit count the action picked at simulation t must have."""
    if m <= 1:
        return list(range(simulations))
    log2m = int(np.ceil(np.log2(m)))
    seq, visits, considered = [], [0] * m, m
    while len(seq) < simulations:
        extra = max(1, simulations // (log2m * considered))
        for _ in range(extra):
            seq.extend(visits[:considered])
            for i in range(considered):
                visits[i] += 1
        considered = max(2, considered // 2)
    return seq[:simulations]


def visit_multiset(m, simulations):
    """The sorted visit counts of the m considered actions after all `simulations`, as the sequence prescribes."""
    counts = [0] * m
    for cv in sequence_of_considered_visits(m, simulations):
        counts[counts.index(cv)] += 1
    return sorted(counts)


def clean_logit(x):
    x = F(x)
    return x if (x >= -BIG and x <= BIG) else F(0.0)


def clean_noise(x):
    x = F(x)
    return x if (x >= -FLT_MAX and x <= FLT_MAX) else F(0.0)


class GumbelTree:
    """One root's session: begin is the constructor, then `leaf()`, `advance(logits_row, value)`, `result()`.
    expand(pos, a) -> (the position after a, seat 0's reward of that step)."""

    def __init__(self, root: Pos, over: bool, expand: Callable[[Pos, int], tuple], simulations: int, considered: int,
                 gumbel, c_visit: float = 50.0, c_scale: float = 0.1):
        self.n_act = len(root.mask)
        self.expand, self.S, self.m = expand, simulations, considered
        self.c_visit, self.c_scale = F(c_visit), F(c_scale)
        self.gumbel = np.array([clean_noise(x) for x in gumbel], F)
        self.nodes = []
        self.over = over
        self._make(root, 0)
        self.path, self.pending, self.status, self.t = [], 0, 2 if over else 0, 0

    def _make(self, pos, term0):
        n = self.n_act
        self.nodes.append(dict(pos=pos, term0=term0, raw=F(term0) if pos.done else F(0.0), child=[-1] * n,
                               v=np.zeros(n, np.int64), w0=np.zeros(n, F), logit=np.zeros(n, F), p=np.zeros(n, F)))
        return len(self.nodes) - 1

    def leaf(self):
        """(obs, mask, status) of the pending leaf: zeros unless status 0."""
        pos = self.nodes[self.pending]["pos"]
        if self.status != 0:
            return np.zeros_like(self.nodes[0]["pos"].obs), np.zeros(self.n_act, bool), self.status
        return pos.obs, pos.mask, 0

    def _evaluate(self, nd):
        """(N, vmax, sigma [A], pi' [A]) of a node."""
        mask = nd["pos"].mask
        sign = F(1 if nd["pos"].mover == 0 else -1)
        v, w0, p, logit = nd["v"], nd["w0"], nd["p"], nd["logit"]
        total = int(v[mask].sum())
        vmax = int(v[mask].max()) if mask.any() else 0
        on = mask & (v > 0)
        q = np.zeros(self.n_act, F)
        q[on] = (sign * w0[on]) / v[on].astype(F)
        sraw = sign * nd["raw"]
        if total == 0:
            mix = sraw
        else:
            sum_pq = wave_sum(np.where(on, p * q, F(0.0)))
            sum_p = wave_sum(np.where(on, p, F(0.0)))
            mix = (sraw + F(total) * (sum_pq / sum_p)) / F(1 + total)
        cq = np.where(v > 0, q, mix).astype(F)
        sigma, pi = np.zeros(self.n_act, F), np.zeros(self.n_act, F)
        if not mask.any():
            return total, vmax, sigma, pi
        lo, hi = cq[mask].min(), cq[mask].max()
        with np.errstate(over="ignore"):
            scale = (self.c_visit + F(vmax)) * self.c_scale
        scale = scale if scale < BIG else BIG
        span = hi - lo
        sigma[mask] = (scale * (cq[mask] - lo)) / (span if span > F(1e-8) else F(1e-8))
        x = logit + sigma
        ex = np.zeros(self.n_act, F)
        ex[mask] = exp_(x[mask] - x[mask].max())
        pi[mask] = ex[mask] / wave_sum(ex)
        for arr in (cq, sigma, x, ex, pi):
            assert arr.dtype == F
        assert isinstance(mix, np.float32) and isinstance(scale, np.float32)
        return total, vmax, sigma, pi

    def _root_pick(self, total, vmax, sigma, final):
        nd = self.nodes[0]
        mask = nd["pos"].mask
        legal = np.flatnonzero(mask)
        if len(legal) == 0:
            return -1
        cv = vmax if final else sequence_of_considered_visits(min(self.m, len(legal)), self.S)[total]
        lmax = nd["logit"][mask].max()
        with np.errstate(over="ignore"):
            key = (self.gumbel + (nd["logit"] - lmax)) + sigma
        assert key.dtype == F
        best, a = None, -1
        for b in legal:
            if nd["v"][b] == cv and (best is None or key[b] > best):
                best, a = key[b], int(b)
        return a

    def advance(self, logits, value):
        assert self.t <= self.S
        t, self.t = self.t, self.t + 1
        if self.status == 2:
            return
        leaf = self.nodes[self.pending]
        if self.status == 0:
            mask = leaf["pos"].mask
            lg = np.array([clean_logit(x) if ok else F(0.0) for x, ok in zip(logits, mask)], F)
            ex = np.zeros(self.n_act, F)
            ex[mask] = exp_(lg[mask] - lg[mask].max())
            p = np.zeros(self.n_act, F)
            p[mask] = np.maximum(ex[mask] / wave_sum(ex), FLT_MIN)
            leaf["logit"], leaf["p"] = lg, p
            leaf["raw"] = F(1 if leaf["pos"].mover == 0 else -1) * cleanv(value)
            val0 = leaf["raw"]
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
            total, vmax, sigma, pi = self._evaluate(nd)
            if node == 0:
                a = self._root_pick(total, vmax, sigma, False)
            else:
                score = pi - nd["v"].astype(F) / F(1 + total)
                assert score.dtype == F
                best, a = None, -1
                for b in np.flatnonzero(nd["pos"].mask):
                    if best is None or score[b] > best:
                        best, a = score[b], int(b)
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
        """(visits int32 [A], values float32 [A], action, weights float32 [A], nodes)"""
        root = self.nodes[0]
        if self.over:
            zero = np.zeros(self.n_act, F)
            return np.zeros(self.n_act, np.int32), zero, -1, zero.copy(), len(self.nodes)
        visits = root["v"].astype(np.int32)
        sign = F(1 if root["pos"].mover == 0 else -1)
        values = (sign * root["w0"]).astype(F)
        total, vmax, sigma, pi = self._evaluate(root)
        return visits, values, self._root_pick(total, vmax, sigma, True), pi, len(self.nodes)


def stand_in_logits(obs, mask):
    """The stand-in evaluator: (logits float32 [k, A], values float32 [k]) from the bytes of obs and mask through the
    integer hashes of pgx_guided_util.stand_in: legal logits spread over -3 .. 3, illegal ones 0."""
    priors, values = stand_in(obs, mask)
    top = np.maximum(priors.max(1, keepdims=True), F(1e-30))
    logits = np.where(np.asarray(mask, bool), (priors / top) * F(6.0) - F(3.0), F(0.0)).astype(F)
    return np.ascontiguousarray(logits), values


def wild_logits(obs, mask):
    """An evaluator with large-magnitude and tied logits: every legal logit is one of six values, two of them +-1e30
    and one pair equal, picked by the row's hash and the action."""
    priors, values = stand_in(obs, mask)
    palette = np.array([-1e30, -50.0, 0.0, 0.0, 50.0, 1e30], F)
    act = np.arange(priors.shape[1])
    pick = ((values.view(np.uint32)[:, None] >> np.uint32(9)) + act[None, :].astype(np.uint32)) % np.uint32(6)
    logits = np.where(np.asarray(mask, bool), palette[pick], F(0.0)).astype(F)
    return np.ascontiguousarray(logits), values


def gumbel_noise(seed, k, n_act):
    """Gumbel(0, 1) float32 noise [k, A] from numpy's PCG64, as the Python wrapper draws it."""
    return np.random.Generator(np.random.PCG64(seed)).gumbel(size=(k, n_act)).astype(F)
