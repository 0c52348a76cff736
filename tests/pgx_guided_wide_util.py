"""The wide sessions of the PGX guided search (envpool_amd/csrc/pgx_guided.hip.h "Several leaves per launch", DESIGN.md
"PGX guided search: several leaves per launch") restated in Python and numpy, independently of the header: W slots per
root, an advance that answers all pending slots and then descends up to W times with virtual losses.  The tree of one
root is kept here, positions and expansion steps come from the caller, `wscore` is computed in np.float32 operation by
operation."""
from typing import Callable

import numpy as np

from pgx_guided_util import Pos, clean, cleanv

F = np.float32


def wscore(v, w0, p, o, total, sign, c_puct):
    """wscore(node, a) of the contract; every operation rounds to float32."""
    n = int(v) + int(o)
    q = (F(sign) * F(w0) - F(int(o))) / F(n) if n > 0 else F(0.0)
    u = (F(c_puct) * F(p)) * np.sqrt(F(int(total) + 1))
    out = q + u / F(1 + n)
    assert isinstance(out, np.float32)
    return out


class WideTree:
    """One root's wide session: begin is the constructor, then `leaves()`, `advance(priors [W, A], values [W])`,
    `result()`, `reroot(a, s2)`.  expand(pos, a) -> (the position after a, seat 0's reward of that step)."""

    def __init__(self, root: Pos, over: bool, expand: Callable[[Pos, int], tuple], simulations: int, c_puct: float,
                 width: int, capacity: int = 0):
        self.n_act = len(root.mask)
        self.expand, self.S, self.c, self.W = expand, simulations, c_puct, width
        self.C = capacity or simulations + 1
        self.nodes = []
        self.over = over
        self._make(root, 0)
        self._idle_slots()
        if not over:
            self.slots[0] = dict(pending=0, path=[], status=0)
        self.done, self.t = 0, 0
        self.collisions = 0

    def _idle_slots(self):
        self.slots = [dict(pending=0, path=[], status=2) for _ in range(self.W)]

    def _make(self, pos, term0):
        n = self.n_act
        self.nodes.append(dict(pos=pos, term0=term0, child=[-1] * n, v=[0] * n, w0=[F(0.0)] * n, p=[F(0.0)] * n))
        return len(self.nodes) - 1

    def leaves(self):
        """(obs [W, ...], mask [W, A], status [W]) of the slots: zeros unless status 0."""
        root = self.nodes[0]["pos"]
        obs = np.zeros((self.W,) + root.obs.shape, bool)
        mask = np.zeros((self.W, self.n_act), bool)
        status = np.array([s["status"] for s in self.slots], np.uint8)
        for j, s in enumerate(self.slots):
            if s["status"] == 0:
                obs[j], mask[j] = self.nodes[s["pending"]]["pos"].obs, self.nodes[s["pending"]]["pos"].mask
        return obs, mask, status

    def advance(self, priors, values):
        assert self.t <= self.S
        self.t += 1
        # A. the answers
        for j, s in enumerate(self.slots):
            if s["status"] == 2:
                continue
            leaf = self.nodes[s["pending"]]
            if s["status"] == 0:
                leaf["p"] = [clean(x) for x in priors[j]]
                val0 = F(1 if leaf["pos"].mover == 0 else -1) * cleanv(values[j])
            else:
                val0 = F(leaf["term0"])
            for n, a in s["path"]:
                self.nodes[n]["v"][a] += 1
                self.nodes[n]["w0"][a] = F(self.nodes[n]["w0"][a] + val0)
            if s["path"]:
                self.done += 1
            s["status"], s["path"] = 2, []
        if self.over:
            return
        # B. the descents
        for j in range(self.W):
            if not (self.done + j < self.S and len(self.nodes) < self.C):
                break
            earlier = self.slots[:j]
            node, path, collided = 0, [], False
            while True:
                nd, d = self.nodes[node], len(path)
                o = [0] * self.n_act
                for e in earlier:
                    if len(e["path"]) > d and e["path"][d][0] == node:
                        o[e["path"][d][1]] += 1
                total = sum(nd["v"]) + sum(o)
                sign = 1 if nd["pos"].mover == 0 else -1
                best, a = None, -1
                for b in np.flatnonzero(nd["pos"].mask):
                    sc = wscore(nd["v"][b], nd["w0"][b], nd["p"][b], o[b], total, sign, self.c)
                    if best is None or sc > best:
                        best, a = sc, int(b)
                assert a >= 0
                path.append((node, a))
                if nd["child"][a] < 0:
                    pos, term0 = self.expand(nd["pos"], a)
                    node = nd["child"][a] = self._make(pos, term0)
                    break
                node = nd["child"][a]
                if self.nodes[node]["pos"].done:
                    break
                if any(e["status"] == 0 and e["pending"] == node for e in earlier):
                    collided = True
                    break
            if collided:
                self.collisions += 1
                break
            self.slots[j] = dict(pending=node, path=path, status=1 if self.nodes[node]["pos"].done else 0)
        assert len(self.nodes) <= self.C
        live = [s["pending"] for s in self.slots if s["status"] == 0]
        assert len(live) == len(set(live))  # no two status-0 slots share a node

    def result(self):
        """(visits int32 [A], values float32 [A], action, nodes, done)"""
        root = self.nodes[0]
        if self.over:
            return np.zeros(self.n_act, np.int32), np.zeros(self.n_act, F), -1, len(self.nodes), self.done
        visits = np.array(root["v"], np.int32)
        sign = F(1 if root["pos"].mover == 0 else -1)
        values = np.array([sign * F(w) for w in root["w0"]], F)
        legal = np.flatnonzero(root["pos"].mask)
        return visits, values, int(legal[np.argmax(visits[legal])]), len(self.nodes), self.done

    def reroot(self, a, s2):
        """The subtree under the played move `a` becomes the tree (kept nodes in their old order); slot 0 holds the new
        root, the other slots are idle whatever they held."""
        self.S, self.t, self.done = s2, 0, 0
        self._idle_slots()
        if self.over:
            return
        root = self.nodes[0]
        c = root["child"][a]
        if c < 0:
            pos, term0 = self.expand(root["pos"], a)
            self.nodes = []
            self._make(pos, term0)
        else:
            keep, stack = set(), [c]
            while stack:
                k = stack.pop()
                keep.add(k)
                stack.extend(ch for ch in self.nodes[k]["child"] if ch >= 0)
            order = sorted(keep)
            new = {old: i for i, old in enumerate(order)}
            kept = []
            for old in order:
                nd = self.nodes[old]
                kept.append(dict(nd, child=[new[ch] if ch >= 0 else -1 for ch in nd["child"]]))
            self.nodes = kept
        if self.nodes[0]["pos"].done:
            self.over = True
        else:
            self.slots[0] = dict(pending=0, path=[], status=0)
