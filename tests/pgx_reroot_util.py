"""Tree reuse of the PGX guided search (envpool_amd/csrc/pgx_guided.hip.h "Tree reuse") restated in Python on top of
pgx_guided_util, independently of the header: the tree of one root is a POINTER tree here -- a node holds its children
as objects --, so reroot just takes the child and no node index exists that a pick could depend on; the node count is
the size of the tree.  Scores, clean / cleanv and the stand-in evaluator are pgx_guided_util's."""
from typing import Callable

import numpy as np

from pgx_guided_util import F, Pos, clean, cleanv, score


class _Node:
    def __init__(self, pos: Pos, term0: int, n_act: int):
        self.pos, self.term0 = pos, term0
        self.child = {}
        self.v = [0] * n_act
        self.w0 = [F(0.0)] * n_act
        self.p = [F(0.0)] * n_act

    def size(self):
        return 1 + sum(c.size() for c in self.child.values())


class RerootTree:
    """One root's session with a node capacity: begin is the constructor, then `leaf()`, `advance(priors_row, value)`,
    `result()` and, after the round's last advance, `reroot(a, simulations)`.
    expand(pos, a) -> (the position after a, seat 0's reward of that step)."""

    def __init__(self, root: Pos, over: bool, expand: Callable[[Pos, int], tuple], simulations: int, c_puct: float,
                 nodes: int = 0):
        self.n_act = len(root.mask)
        self.expand, self.S, self.c = expand, simulations, c_puct
        self.C = nodes or simulations + 1
        assert simulations + 1 <= self.C
        self.over = over
        self.root = _Node(root, 0, self.n_act)
        self.count = 1
        self.path, self.pending, self.status, self.t = [], self.root, 2 if over else 0, 0

    def leaf(self):
        """(obs, mask, status) of the pending leaf: zeros unless status 0."""
        if self.status != 0:
            return np.zeros_like(self.root.pos.obs), np.zeros(self.n_act, bool), self.status
        return self.pending.pos.obs, self.pending.pos.mask, 0

    def advance(self, priors, value):
        assert self.t <= self.S
        t, self.t = self.t, self.t + 1
        if self.status == 2:
            return
        leaf = self.pending
        if self.status == 0:
            leaf.p = [clean(x) for x in priors]
            val0 = F(1 if leaf.pos.mover == 0 else -1) * cleanv(value)
        else:
            val0 = F(leaf.term0)
        for n, a in self.path:
            n.v[a] += 1
            n.w0[a] = F(n.w0[a] + val0)
        if t == self.S or self.count >= self.C:  # the last call, or the memory is used up: a normal end
            self.status = 2
            return
        node, self.path = self.root, []
        while True:
            total = sum(node.v)
            sign = 1 if node.pos.mover == 0 else -1
            best, a = None, -1
            for b in np.flatnonzero(node.pos.mask):
                s = score(node.v[b], node.w0[b], node.p[b], total, sign, self.c)
                if best is None or s > best:
                    best, a = s, int(b)
            assert a >= 0
            self.path.append((node, a))
            if a not in node.child:
                pos, term0 = self.expand(node.pos, a)
                node.child[a] = node = _Node(pos, term0, self.n_act)
                self.count += 1
                break
            node = node.child[a]
            if node.pos.done:
                break
        self.pending = node
        self.status = 1 if node.pos.done else 0
        assert self.count <= self.C

    def result(self):
        """(visits int32 [A], values float32 [A], action, nodes)"""
        root = self.root
        if self.over:
            return np.zeros(self.n_act, np.int32), np.zeros(self.n_act, F), -1, self.count
        visits = np.array(root.v, np.int32)
        sign = F(1 if root.pos.mover == 0 else -1)
        values = np.array([sign * F(w) for w in root.w0], F)
        legal = np.flatnonzero(root.pos.mask)
        return visits, values, int(legal[np.argmax(visits[legal])]), self.count

    def reroot(self, a, simulations=None):
        assert self.t == self.S + 1, "the round is not complete"
        self.S = self.S if simulations is None else simulations
        assert 1 <= self.S and self.S + 1 <= self.C
        self.t, self.path = 0, []
        if self.over:  # an idle root stays over; a is ignored
            self.status = 2
            return
        if not 0 <= a < self.n_act:
            self.over, self.status = True, 2
            return
        if a in self.root.child:
            self.root = self.root.child[a]
            self.count = self.root.size()
        else:
            pos, term0 = self.expand(self.root.pos, a)
            self.root = _Node(pos, term0, self.n_act)
            self.count = 1
        self.pending = self.root
        self.over = bool(self.root.pos.done)
        self.status = 2 if self.over else 0
