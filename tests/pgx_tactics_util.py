"""Shared helpers of the tests of the PGX guided search's exact leaf status (envpool_amd/csrc/pgx_guided.hip.h "Exact
leaf status"): the g++ harness, positions by their hidden words, the numpy restatements (`GuidedTree` / `WideTree`)
driven through subclasses that decide each new status-0 leaf after the advance's descents with the brute-force minimax
(pgx_solve_brute.cpp, which shares nothing with the solver), the two evaluators, the root sets with their recorded
seeds, and the call-for-call comparison of harness and restatement."""
import ctypes
import os
import subprocess

import numpy as np

from pgx_guided_util import GuidedTree, Pos, stand_in
from pgx_guided_wide_util import WideTree
from pgx_solve_util import brute_solve, hand_made, host_reset
from pgx_util import ACTIONS, CODE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
GAMES = ["TicTacToe", "ConnectFour", "Othello", "Hex"]
SHAPE = {"TicTacToe": (3, 3, 2), "ConnectFour": (6, 7, 2), "Hex": (11, 11, 4), "Othello": (8, 8, 2)}
C_PUCT = 1.25
BIG = 1 << 20  # the largest tactics_nodes: nothing of the test shapes is given up
# the shapes: simulations, the width of the wide runs, the horizons, the plies rolled from the reset, and the seed of
# the roll-out (chosen on the CPU with the brute force so that the restatement alone meets the coverage conditions:
# per game a leaf decided +1, one decided -1, an evaluated leaf and a native finished-game leaf)
SIMS = {"TicTacToe": 24, "ConnectFour": 24, "Othello": 16, "Hex": 16}
WIDTH = {"TicTacToe": 4, "ConnectFour": 4, "Othello": 4, "Hex": 2}
DEPTHS = {"TicTacToe": [1, 2, 3], "ConnectFour": [1, 2, 4], "Othello": [2, 3], "Hex": [1, 2]}
PLIES = {"TicTacToe": 3, "ConnectFour": 10, "Othello": 50}
ROLL_SEED = {"TicTacToe": 1, "ConnectFour": 19, "Othello": 1}
ROLLED = 8
# Othello 50 plies in has about ten empty squares: no leaf of a 16-simulation search is within 3 plies of the end, so
# nothing there is decided.  Two more roots 56 plies in (seed 18) bring the decided and the native finished leaves.
OTHELLO_LATE = (2, 56, 18)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def compile_harness(tmp, source, flags=(), shared=True):
    out = str(tmp / (("lib" + source.replace(".cpp", ".so")) if shared else source.replace(".cpp", "")))
    kind = ["-shared", "-fPIC"] if shared else []
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *kind, *flags,
                    os.path.join(ROOT, "tests", "cpu_harness", source), "-o", out], check=True)
    return out


def build_libs(tmp):
    """{tactics, brute, host}: the harness of this feature (with the wide harness's entry points), the brute-force
    minimax, the replay harness (for the reset positions)."""
    libs = {k: ctypes.CDLL(compile_harness(tmp, src)) for k, src in
            (("tactics", "pgx_tactics_host.cpp"), ("brute", "pgx_solve_brute.cpp"), ("host", "pgx_host.cpp"))}
    t = libs["tactics"]
    t.pgx_tactics_begin.restype = ctypes.c_void_p
    t.pgx_wide_begin.restype = ctypes.c_void_p
    t.pgx_tactics_decided.restype = None
    t.pgx_wide_result.restype = None
    t.pgx_wide_end.restype = None
    return libs


class Game:
    """Positions of one game by their hidden words: `pos`, `expand` (for the restatements) and `decide` (the brute
    force's verdict on a leaf)."""

    def __init__(self, libs, fam):
        self.fam, self.code, self.lib, self.brute = fam, CODE[fam], libs["tactics"], libs["brute"]
        self.n_act = ACTIONS[fam]
        self.brute_calls = 0

    def step(self, hid, action):
        hid = np.ascontiguousarray(hid, np.int32)
        out, info = np.zeros_like(hid), np.zeros(4, np.int32)
        obs, mask = np.zeros(SHAPE[self.fam], np.uint8), np.zeros(self.n_act, np.uint8)
        assert self.lib.pgx_tactics_step(self.code, _ptr(hid), int(action), _ptr(out), _ptr(obs), _ptr(mask),
                                         _ptr(info)) == 0
        pos = Pos(mask=mask.astype(bool), done=bool(info[0]), mover=int(info[1]), obs=obs.astype(bool), key=(None, out))
        assert info[2] == -info[3]  # zero-sum
        return pos, int(info[2])

    def pos(self, hid, done=False):
        return self.step(hid, -1)[0]._replace(done=bool(done))

    def expand(self, pos, a):
        assert pos.mask[a] and not pos.done
        return self.step(pos.key[1], a)

    def decide(self, pos, depth):
        """v != 0: the position is a forced win (+1) or loss (-1) for its mover within `depth` plies; else 0."""
        self.brute_calls += 1
        (value, _, _, status), _ = brute_solve(self.brute, self.fam, pos.key[1][None], [0], depth)
        assert status[0] == 0
        return int(value[0])


class _Tally:
    """What the coverage conditions count, and the exact part of the root's values."""

    def tally_init(self, game, depth):
        self.game, self.D = game, depth
        self.decided = 0
        self.events = {"+1": 0, "-1": 0, "eval": 0, "native": 0}
        self.exact = np.zeros(self.n_act, F)  # per root action: the decided and finished results backed up through it

    def answered(self, status, pending, path):
        if status == 1 and path:
            sign = 1 if self.nodes[0]["pos"].mover == 0 else -1
            self.exact[path[0][1]] += F(sign * self.nodes[pending]["term0"])

    def look_at(self, status, pending):
        """The stage after the descents for one slot; returns the slot's status."""
        node = self.nodes[pending]
        if status == 1 and not node.get("decided"):
            self.events["native"] += 1
        if status != 0 or pending == 0:
            return status
        v = self.game.decide(node["pos"], self.D) if self.D else 0
        if v == 0:
            self.events["eval"] += 1
            return 0
        node["open"] = node["pos"]
        node["pos"] = node["pos"]._replace(done=True)  # from now on a finished game ...
        node["term0"] = (1 if node["open"].mover == 0 else -1) * v  # ... whose last reward is v for its mover
        node["decided"] = True
        self.decided += 1
        self.events["+1" if v > 0 else "-1"] += 1
        return 1


class TacticsGuidedTree(GuidedTree, _Tally):
    """The plain restatement with the exact leaf status."""

    def __init__(self, game, root, simulations, depth):
        GuidedTree.__init__(self, root, root.done, game.expand, simulations, C_PUCT)
        self.tally_init(game, depth)

    def advance(self, priors, value):
        self.answered(self.status, self.pending, self.path)
        was = self.status
        GuidedTree.advance(self, priors, value)
        if self.status != 2 and was != 2:
            self.status = self.look_at(self.status, self.pending)


class TacticsWideTree(WideTree, _Tally):
    """The wide restatement with the exact leaf status, and reroot's rule 5."""

    def __init__(self, game, root, simulations, width, depth, capacity=0):
        WideTree.__init__(self, root, root.done, game.expand, simulations, C_PUCT, width, capacity)
        self.tally_init(game, depth)

    def advance(self, priors, values):
        for s in self.slots:
            self.answered(s["status"], s["pending"], s["path"])
        WideTree.advance(self, priors, values)
        for s in self.slots:  # after ALL descents of the launch
            if s["status"] != 2:
                s["status"] = self.look_at(s["status"], s["pending"])

    def reroot(self, a, s2):
        c = -1 if self.over else self.nodes[0]["child"][a]
        if c >= 0 and self.nodes[c].get("decided"):  # the game runs on; term0 stays and is not used
            self.nodes[c]["pos"], self.nodes[c]["decided"] = self.nodes[c]["open"], False
        WideTree.reroot(self, a, s2)


def stand_in_rows(obs, mask):
    lead = mask.shape[:-1]
    priors, values = stand_in(obs.reshape((-1,) + obs.shape[len(lead):]), mask.reshape(-1, mask.shape[-1]))
    return priors.reshape(lead + (-1,)), values.reshape(lead)


def constant_rows(obs, mask):
    """The constant evaluator: uniform priors over the legal actions, value 0."""
    m = np.asarray(mask).astype(F)
    priors = m / np.maximum(m.sum(-1, keepdims=True), F(1)).astype(F)
    return np.ascontiguousarray(priors, F), np.zeros(mask.shape[:-1], F)


EVALUATORS = {"stand_in": stand_in_rows, "constant": constant_rows}


class TacticsHost:
    """The harness's session over positions (Pos with key[1] = hidden words); leaf arrays [n, W, ...]."""

    def __init__(self, libs, fam, poss, simulations, width, tactics, tactics_nodes=BIG, nodes=0, want_rc=0, plain=None):
        self.lib, self.n, self.n_act, self.W = libs["tactics"], len(poss), ACTIONS[fam], width
        hid = np.ascontiguousarray(np.stack([p.key[1] for p in poss]), np.int32)
        done = np.array([p.done for p in poss], np.uint8)
        w = max(width, 1)
        self.obs = np.full((self.n, w) + SHAPE[fam], 7, np.uint8)
        self.mask = np.full((self.n, w, self.n_act), 7, np.uint8)
        self.status = np.full((self.n, w), 7, np.uint8)
        rc = ctypes.c_int(-9)
        args = (CODE[fam], self.n, _ptr(hid), _ptr(done), simulations, nodes or simulations + 1, width,
                ctypes.c_float(C_PUCT))
        tail = (_ptr(self.obs), _ptr(self.mask), _ptr(self.status), ctypes.byref(rc))
        if plain:  # the wide harness's own begin: a session that knows nothing of tactics
            self.h = self.lib.pgx_wide_begin(*args, *tail)
        else:
            self.h = self.lib.pgx_tactics_begin(*args, int(tactics), ctypes.c_longlong(int(tactics_nodes)), *tail)
        assert rc.value == want_rc and bool(self.h) == (want_rc == 0)
        self.tactics = not plain

    def leaves(self):
        return self.obs.copy(), self.mask.copy(), self.status.copy()

    def advance(self, priors, values):
        priors, values = np.ascontiguousarray(priors, F), np.ascontiguousarray(values, F)
        assert priors.shape == (self.n, self.W, self.n_act) and values.shape == (self.n, self.W)
        return self.lib.pgx_wide_advance(ctypes.c_void_p(self.h), _ptr(priors), _ptr(values), _ptr(self.obs),
                                         _ptr(self.mask), _ptr(self.status))

    def result(self):
        visits, values = np.full((self.n, self.n_act), -7, np.int32), np.full((self.n, self.n_act), -7, F)
        action, nodes, done = np.full(self.n, -7, np.int32), np.zeros(self.n, np.int32), np.zeros(self.n, np.int32)
        self.lib.pgx_wide_result(ctypes.c_void_p(self.h), _ptr(visits), _ptr(values), _ptr(action), _ptr(nodes),
                                 _ptr(done))
        return visits, values, action, nodes, done

    def decided(self):
        """(decided [n], the solver's positions [n], given up in the last advance [n, W])"""
        d, nodes = np.full(self.n, -7, np.int32), np.full(self.n, -7, np.int64)
        gave_up = np.zeros((self.n, self.W), np.uint8)
        self.lib.pgx_tactics_decided(ctypes.c_void_p(self.h), _ptr(d), _ptr(nodes), _ptr(gave_up))
        return d, nodes, gave_up

    def reroot(self, actions, s2):
        actions = np.ascontiguousarray(actions, np.int32)
        return self.lib.pgx_wide_reroot(ctypes.c_void_p(self.h), _ptr(actions), s2, _ptr(self.obs), _ptr(self.mask),
                                        _ptr(self.status))

    def close(self):
        self.lib.pgx_wide_end(ctypes.c_void_p(self.h))
        self.h = None


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


class Pair:
    """The harness's session over `roots` and one restatement per root, fed the same rows and compared call for call:
    status, obs, mask, the result (visits, values bit for bit, action) and decided."""

    def __init__(self, libs, game, roots, simulations, width, depth, evaluator, nodes=0, wide_tree=None):
        self.game, self.roots, self.S, self.W, self.D = game, roots, simulations, width, depth
        self.fed = EVALUATORS[evaluator]
        self.constant = evaluator == "constant"
        self.host = TacticsHost(libs, game.fam, roots, simulations, width, depth, BIG, nodes)
        if wide_tree is None:
            wide_tree = width > 1 or nodes != 0
        self.wide_tree = wide_tree
        if wide_tree:
            self.trees = [TacticsWideTree(game, r, simulations, width, depth, nodes or simulations + 1) for r in roots]
        else:
            self.trees = [TacticsGuidedTree(game, r, simulations, depth) for r in roots]
        self.calls = 0

    def tree_leaves(self, tree):
        if self.wide_tree:
            return tree.leaves()
        obs, mask, status = tree.leaf()
        return obs[None], mask[None], np.array([status], np.uint8)

    def same_leaves(self, what):
        obs, mask, status = self.host.leaves()
        for i, tree in enumerate(self.trees):
            want = self.tree_leaves(tree)
            assert np.array_equal(status[i], want[2]), (self.game.fam, what, i, status[i], want[2])
            assert np.array_equal(obs[i].astype(bool), want[0]) and np.array_equal(mask[i].astype(bool), want[1]), what
        assert set(np.unique(obs)) <= {0, 1} and set(np.unique(mask)) <= {0, 1}
        idle = status != 0
        assert not obs[idle].any() and not mask[idle].any()
        return obs, mask, status

    def same_result(self, what):
        got = self.host.result()
        decided = self.host.decided()[0]
        for i, tree in enumerate(self.trees):
            ref = tree.result()
            assert np.array_equal(got[0][i], ref[0]), (self.game.fam, what, i, got[0][i], ref[0])
            assert np.array_equal(bits(got[1][i]), bits(ref[1])), (self.game.fam, what, i, got[1][i], ref[1])
            assert got[2][i] == ref[2] and got[3][i] == ref[3], (what, i)
            assert decided[i] == tree.decided, (self.game.fam, what, i, decided[i], tree.decided)
            if self.constant:  # the root's values are exactly the decided and finished results through each action
                assert np.array_equal(bits(got[1][i] + F(0)), bits(tree.exact + F(0))), (what, i, got[1][i], tree.exact)
        return got

    def round(self):
        t = 0
        while True:
            obs, mask, status = self.same_leaves(t)
            if (status == 2).all():
                break
            assert t <= self.S, "a round is complete after at most S + 1 advances"
            priors, values = self.fed(obs, mask)
            priors[status == 1] = 1e30  # whatever the caller says in a row of status 1 is ignored
            values[status == 1] = 1.0 if t % 2 else -1.0
            assert self.host.advance(priors, values) == 0
            for i, tree in enumerate(self.trees):
                if self.wide_tree:
                    tree.advance(priors[i], values[i])
                else:
                    tree.advance(priors[i, 0], values[i, 0])
            self.same_result(t)
            t += 1
        self.calls = t
        return self.host.result()

    def reroot(self, actions, s2=None):
        s2 = s2 or self.S
        assert self.host.reroot(actions, s2) == 0
        for tree, a in zip(self.trees, actions):
            tree.reroot(int(a), s2)
        self.S = s2
        self.same_leaves("reroot")
        self.same_result("reroot")

    def events(self):
        out = {"+1": 0, "-1": 0, "eval": 0, "native": 0}
        for tree in self.trees:
            for k, v in tree.events.items():
                out[k] += v
        return out

    def close(self):
        self.host.close()


# ---- the root sets --------------------------------------------------------------------------------------------------
def rolled_roots(libs, game, n, plies, seed):
    """n roots `plies` seeded random legal plies from their resets (a game that ends earlier stops one ply before)."""
    hid, _ = host_reset(libs["host"], game.fam, n, 11)
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        pos = game.pos(hid[i])
        for _ in range(plies):
            nxt, _ = game.expand(pos, int(rng.choice(np.flatnonzero(pos.mask))))
            if nxt.done:
                break
            pos = nxt
        out.append(pos)
    return out


def over_root(game, pos):
    """A root that is over at begin: the position of `pos`, marked done as an env's done flag marks it."""
    return pos._replace(done=True)


def _hex_words(mine, theirs, turn, cp):
    """Hex hidden words: the board as the side to move sees it (1 its own stones, -1 the other's), the turn (even:
    color 0, which joins x = 0 to x = 10, is to move; cell (x, y) is x * 11 + y), the seat of color 0."""
    w = np.zeros(123, np.int32)
    w[list(mine)] = 1
    w[list(theirs)] = -1
    w[121], w[122] = turn, cp
    return w


def single_move_root(libs, game):
    """A running root with a single legal move (for W > 1: idle slots, collisions, several slots on one finished game).
      TicTacToe    one empty cell
      ConnectFour  six full columns, found by seeded random play
      Othello      the first position of seeded random play with one legal move
      Hex          row y = 5 of color 0 but for (5, 5), every other cell color 1: (5, 5) is the one empty cell, neither
                   side is connected, and whoever plays there wins (no position of a real game, but one of the
                   rules')"""
    fam = game.fam
    if fam == "Hex":
        row = [x * 11 + 5 for x in range(11) if x != 5]
        rest = [c for c in range(121) if c not in row and c != 60]
        pos = game.pos(_hex_words(row, rest, 120, 0))
        assert pos.mask.sum() == 1 and pos.mask[60]
        return pos
    hid, _ = host_reset(libs["host"], fam, 1, 11)
    rng = np.random.default_rng(5)
    for _ in range(2000):
        pos = game.pos(hid[0])
        while not pos.done:
            if pos.mask.sum() == 1:
                return pos
            pos, _ = game.expand(pos, int(rng.choice(np.flatnonzero(pos.mask))))
    raise AssertionError("no single-move root found")


def hex_roots(game):
    """The hand-made chain positions (pgx_solve_util.hand_made) with the last 2 stones removed, in two ways each: the
    last stone of either colour, and the last two of the edge colour -- so that the chain's owner is one, two and three
    plies from its win and the leaves below come out decided +1, decided -1 and undecided at D = 1 and 2."""
    chain9, edge9 = [x * 11 + 5 for x in range(9)], [x * 11 for x in range(9)]
    chain10 = chain9 + [9 * 11 + 5]
    return [game.pos(w) for w in (
        _hex_words(chain9[:-1], edge9[:-1], 16, 0),   # `win` less (8, 5) and (8, 0): color 0 to move, chain 0..7
        _hex_words(chain9, edge9[:-2], 16, 0),        # `win` less (7, 0) and (8, 0): color 0 to move, chain 0..8
        _hex_words(edge9[:-1], chain10[:-1], 17, 1),  # `loss` less (9, 5) and (8, 0): color 1 to move, chain 0..8
        _hex_words(edge9[:-2], chain10, 17, 1),       # `loss` less (7, 0) and (8, 0): color 1 to move, chain 0..9
        # a fifth, for the coverage: `loss` less (8, 0) alone, color 0 to move with the chain 0..9 -- two moves win at
        # once (native finished leaves) and after any other the reply is lost in 2 (decided -1 at D = 2)
        _hex_words(chain10, edge9[:-1], 18, 1),
    )]


def root_set(libs, game, width=1):
    """The roots of one game's tests: the rolled or hand-made ones, one that is over at begin, and one with a single
    legal move."""
    fam = game.fam
    if fam == "Hex":
        assert [int(w[-2]) for w, _, _, _ in hand_made("Hex")] == [18, 19]  # (the positions hex_roots starts from)
        roots = hex_roots(game)
    else:
        roots = rolled_roots(libs, game, ROLLED, PLIES[fam], ROLL_SEED[fam])
        if fam == "Othello":
            roots += rolled_roots(libs, game, *OTHELLO_LATE)
    return roots + [over_root(game, roots[0]), single_move_root(libs, game)]
