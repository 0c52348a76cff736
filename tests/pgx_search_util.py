"""The PGX tree search (envpool_amd/csrc/pgx_search.hip.h, DESIGN.md "PGX search") restated in Python and numpy,
independently of the header: the tree is kept here, positions, expansion steps and leaf values come from the caller
(the reference-pinned replay and the playout harness on the CPU, public pool calls on the GPU), scores are computed in
np.float32 operation by operation."""
from typing import Any, Callable, NamedTuple

import numpy as np


class Pos(NamedTuple):
    """A position as the search sees it."""

    mask: np.ndarray  # bool [A]: info:legal_action_mask
    done: bool
    mover: int        # info:current_player
    key: Any          # whatever the caller's expand / leaf need to find the position again


def score(v, w0, total, sign, r, c_puct):
    """score(node, a) of the contract; every operation rounds to float32."""
    f = np.float32
    q = f(sign * int(w0)) / f(int(v) * r) if v > 0 else f(0.0)
    u = f(c_puct) * np.sqrt(f(int(total)))
    out = q + u / f(1 + int(v))
    assert isinstance(out, np.float32)
    return out


def puct_search(root: Pos, expand: Callable[[Pos, int], tuple], leaf: Callable[[Pos, int], int], simulations: int,
                leaf_playouts: int, c_puct: float):
    """expand(pos, a) -> (the position after a, seat 0's reward of that step); leaf(pos, t) -> the sum of seat 0's
    returns of the leaf playouts of simulation t from pos.  Returns (visits [A], returns [A], action, nodes)."""
    n_act = len(root.mask)
    if root.done:
        return np.zeros(n_act, np.int32), np.zeros(n_act, np.int32), -1, 0
    nodes = []

    def make(pos, term0):
        nodes.append(dict(pos=pos, term0=term0, child=[-1] * n_act, v=[0] * n_act, w0=[0] * n_act))
        return len(nodes) - 1

    make(root, 0)
    for t in range(simulations):
        node, path = 0, []
        while True:
            nd = nodes[node]
            if nd["pos"].done:
                val0 = leaf_playouts * nd["term0"]
                break
            total = sum(nd["v"])
            sign = 1 if nd["pos"].mover == 0 else -1
            best, a = None, -1
            for b in np.flatnonzero(nd["pos"].mask):
                s = score(nd["v"][b], nd["w0"][b], total, sign, leaf_playouts, c_puct)
                if best is None or s > best:
                    best, a = s, int(b)
            path.append((node, a))
            if nd["child"][a] < 0:
                pos, term0 = expand(nd["pos"], a)
                nd["child"][a] = make(pos, term0)
                val0 = leaf_playouts * term0 if pos.done else leaf(pos, t)
                break
            node = nd["child"][a]
        for n, a in path:
            nodes[n]["v"][a] += 1
            nodes[n]["w0"][a] += val0
    assert len(nodes) <= simulations + 1
    visits = np.array(nodes[0]["v"], np.int32)
    sign = 1 if root.mover == 0 else -1
    returns = (sign * np.array(nodes[0]["w0"], np.int64)).astype(np.int32)
    legal = np.flatnonzero(root.mask)
    return visits, returns, int(legal[np.argmax(visits[legal])]), len(nodes)
