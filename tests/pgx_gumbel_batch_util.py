"""The batch sessions of the PGX Gumbel search (envpool_amd/csrc/pgx_gumbel.hip.h "A level per launch", DESIGN.md "PGX
Gumbel search: a level per launch") restated in Python and numpy float32, independently of the header: one root's tree
with its B slots, on top of GumbelTree of pgx_gumbel_util.py, whose node arithmetic (sigma, pi', the exponential, the
wave's order of summation) it reuses.  The level of a simulation is read off the SEQUENCE form of sequential halving;
the header walks the table in integers instead."""
import numpy as np

from pgx_guided_util import cleanv
from pgx_gumbel_util import FLT_MIN, GumbelTree, clean_logit, exp_, sequence_of_considered_visits, wave_sum

F = np.float32


def level_left(m, simulations, t):
    """What is left of the level of simulation t: the number of t' in t .. S-1 whose considered visit count is t's."""
    seq = sequence_of_considered_visits(m, simulations)
    return sum(1 for cv in seq[t:] if cv == seq[t])


def levels(m, simulations):
    """The sizes of the levels of a round, in order."""
    out, t = [], 0
    while t < simulations:
        out.append(level_left(m, simulations, t))
        t += out[-1]
    return out


def advances_of_a_round(m_eff, simulations, batch):
    """The advances a root of m_eff considered actions takes until all its statuses are 2."""
    return 1 + sum(-(-size // batch) for size in levels(m_eff, simulations))


class GumbelBatchTree(GumbelTree):
    """One root's batch session: begin is the constructor, then `leaves()`, `advance(logits [B, A], values [B])`,
    `result()` (the plain result: one row).  A slot is {pending, path, status}."""

    def __init__(self, root, over, expand, simulations, considered, batch, gumbel, **consts):
        super().__init__(root, over, expand, simulations, considered, gumbel, **consts)
        self.B = batch
        self.slots = [dict(pending=0, path=[], status=2 if (over or j > 0) else 0) for j in range(batch)]
        self.broken = False

    def leaves(self):
        """[(obs, mask, status)] per slot: zeros unless status 0."""
        root = self.nodes[0]["pos"]
        out = []
        for sl in self.slots:
            pos = self.nodes[sl["pending"]]["pos"]
            if sl["status"] != 0:
                out.append((np.zeros_like(root.obs), np.zeros(self.n_act, bool), sl["status"]))
            else:
                out.append((pos.obs, pos.mask, 0))
        return out

    def _answer(self, sl, logits, value):
        leaf = self.nodes[sl["pending"]]
        if sl["status"] == 0:
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
        for n, a in sl["path"]:
            self.nodes[n]["v"][a] += 1
            self.nodes[n]["w0"][a] = F(self.nodes[n]["w0"][a] + val0)
        sl["status"], sl["path"] = 2, []

    def _descend(self, a):
        """The descent through root action a: (path, pending node)."""
        node, path = 0, []
        while True:
            nd = self.nodes[node]
            path.append((node, a))
            if nd["child"][a] < 0:
                pos, term0 = self.expand(nd["pos"], a)
                node = nd["child"][a] = self._make(pos, term0)
                break
            node = nd["child"][a]
            nd = self.nodes[node]
            if nd["pos"].done:
                break
            total, _, _, pi = self._evaluate(nd)
            score = pi - nd["v"].astype(F) / F(1 + total)
            assert score.dtype == F
            best, a = None, -1
            for b in np.flatnonzero(nd["pos"].mask):
                if best is None or score[b] > best:
                    best, a = score[b], int(b)
            assert a >= 0
        return path, node

    def advance(self, logits, values):
        assert self.t <= self.S
        self.t += 1
        for j, sl in enumerate(self.slots):
            if sl["status"] != 2:
                self._answer(sl, logits[j], values[j])
        if self.over or self.broken:
            return
        root = self.nodes[0]
        mask = root["pos"].mask
        total, _, sigma, _ = self._evaluate(root)
        if total >= self.S:
            return
        legal = np.flatnonzero(mask)
        m_eff = min(self.m, len(legal))
        cv = sequence_of_considered_visits(m_eff, self.S)[total]
        b = min(self.B, level_left(m_eff, self.S, total))
        lmax = root["logit"][mask].max()
        with np.errstate(over="ignore"):
            key = (self.gumbel + (root["logit"] - lmax)) + sigma
        assert key.dtype == F
        cand = [int(a) for a in legal if root["v"][a] == cv]
        chosen = []
        for _ in range(b):  # b arg-max rounds, each without the winners before it; ties: the lowest a
            best, pick = None, -1
            for a in cand:
                if a not in chosen and (best is None or key[a] > best):
                    best, pick = key[a], a
            if pick < 0:
                break
            chosen.append(pick)
        if not chosen:
            self.broken = True
            return
        for j, a in enumerate(chosen):
            path, node = self._descend(a)
            self.slots[j].update(pending=node, path=path, status=1 if self.nodes[node]["pos"].done else 0)
        assert len(self.nodes) <= self.S + 1
