"""Shared helpers of the tests of the PGX guided search's proven values (envpool_amd/csrc/pgx_guided.hip.h "Proven
values"): the g++ harness (pgx_prove_host.cpp, which carries the tactics harness's entry points), the numpy
restatements of rules 1 .. 9 as subclasses of the tactics restatements (whose leaves the brute-force minimax decides) --
they share nothing with the header but the contract's text --, the root sets, the call-for-call comparison, and the
brute force's full solve of a root as the independent truth."""
import ctypes

import numpy as np

import pgx_tactics_util as tu
from pgx_guided_util import clean, cleanv, score
from pgx_guided_wide_util import wscore
from pgx_solve_util import brute_solve, host_reset
from pgx_tactics_util import (BIG, C_PUCT, F, SHAPE, Game, Pair, TacticsGuidedTree, TacticsHost, TacticsWideTree,
                              _hex_words, _ptr, compile_harness, over_root, single_move_root)
from pgx_util import ACTIONS, CODE

GAMES = ["TicTacToe", "ConnectFour", "Othello", "Hex"]
UNPROVEN = -128
PROVE = 1
# the shapes (chosen on the CPU so that the restatement alone meets the coverage conditions of test_pgx_prove_host.py):
# simulations, the plies rolled from the reset and the seed of the roll-out.  The roots are late enough for the brute
# force to solve them to the end: that is the independent truth of every proof.
SIMS = {"TicTacToe": 32, "ConnectFour": 32, "Othello": 32, "Hex": 24}
PLIES = {"TicTacToe": (2, 4), "ConnectFour": (28, 31), "Othello": (50, 53)}
ROLL_SEED = {"TicTacToe": 3, "ConnectFour": 5, "Othello": 7}
ROLLED = 3
OTHELLO_DRAWS = (43, 168)
EVENTS = ("won", "lost", "draw", "early", "pick", "result", "onto", "deeper", "at_once")


def build_libs(tmp):
    """{tactics, brute, host}: this feature's harness under the tactics harness's name (it has all its entry points),
    the brute-force minimax, the replay harness."""
    libs = {k: ctypes.CDLL(compile_harness(tmp, src)) for k, src in
            (("tactics", "pgx_prove_host.cpp"), ("brute", "pgx_solve_brute.cpp"), ("host", "pgx_host.cpp"))}
    t = libs["tactics"]
    for name in ("pgx_prove_begin", "pgx_tactics_begin", "pgx_wide_begin"):
        getattr(t, name).restype = ctypes.c_void_p
    for name in ("pgx_prove_proof", "pgx_tactics_decided", "pgx_wide_result", "pgx_wide_end"):
        getattr(t, name).restype = None
    return libs


# ---- the restatement ------------------------------------------------------------------------------------------------
class _Prove:
    """Rules 1 .. 8 over the nodes of a restatement (dicts with pos, term0, child, v, w0, p).  A proven node is one
    whose pos.done is set: a finished game, a decided leaf or a node marked here; `term0` is its value for seat 0."""

    def prove_init(self):
        self.root_proof = UNPROVEN
        self.seen = dict.fromkeys(EVENTS, 0)

    @staticmethod
    def sign(nd):
        return 1 if nd["pos"].mover == 0 else -1

    def child_value(self, nd, a):
        """rule 1: the proven value of the child of action a for nd's mover"""
        c = nd["child"][a]
        if c < 0 or not self.nodes[c]["pos"].done:
            return UNPROVEN
        return self.sign(nd) * int(self.nodes[c]["term0"])

    def rule2(self, nd):
        vals = [self.child_value(nd, int(a)) for a in np.flatnonzero(nd["pos"].mask)]
        if 1 in vals:
            return 1
        if vals and UNPROVEN not in vals:
            return max(vals)
        return UNPROVEN

    def climb(self, path, pending):
        """rule 3, from a slot of status 1 whose statistics have been backed up"""
        below = pending
        for n, _ in reversed(path):
            if not self.nodes[below]["pos"].done:
                return
            nd = self.nodes[n]
            v = self.rule2(nd)
            if v == UNPROVEN:
                return
            if n == 0:
                assert self.root_proof in (UNPROVEN, v)  # proofs are exact
                if self.root_proof == UNPROVEN and self.done < self.S:
                    self.seen["early"] += 1
                self.root_proof = v
                self.seen["draw"] += v == 0
                return
            if nd.get("decided"):  # marked before: deriving it again gives the same value
                assert nd.get("marked") and nd["term0"] == self.sign(nd) * v
            else:
                vals = [self.child_value(nd, int(a)) for a in np.flatnonzero(nd["pos"].mask)]
                self.seen["won"] += v == 1 and UNPROVEN in vals  # by one child, not by all of them
                self.seen["lost"] += v == -1
                self.seen["draw"] += v == 0
                nd["open"] = nd["pos"]
                nd["pos"] = nd["pos"]._replace(done=True)
                nd["term0"] = self.sign(nd) * v
                nd["decided"] = nd["marked"] = True  # (the tactics restatement's reroot reopens a `decided` node)
            below = n

    def open_actions(self, nd):
        """rule 4: the legal actions a pick chooses among"""
        legal = [int(a) for a in np.flatnonzero(nd["pos"].mask)]
        left = [a for a in legal if self.child_value(nd, a) != -1]
        return left or legal, legal

    def pick(self, nd, key):
        left, legal = self.open_actions(nd)
        best = max(left, key=lambda a: (key(a), -a))
        self.seen["pick"] += best != max(legal, key=lambda a: (key(a), -a))
        return best

    def prove_result(self, out):
        """rule 6 over the plain result tuple"""
        if self.over:
            return out
        root = self.nodes[0]
        legal = [int(a) for a in np.flatnonzero(root["pos"].mask)]
        if self.root_proof != UNPROVEN:
            left = [a for a in legal if self.child_value(root, a) == self.root_proof]
        else:
            left = [a for a in legal if self.child_value(root, a) != -1]
        action = max(left or legal, key=lambda a: (root["v"][a], -a))
        self.differs = action != out[2]
        return out[:2] + (action,) + out[3:]

    def proof(self):
        """rule 7: (value, q int8 [A])"""
        q = np.full(self.n_act, UNPROVEN, np.int8)
        if self.over:
            return UNPROVEN, q
        root = self.nodes[0]
        for a in np.flatnonzero(root["pos"].mask):
            q[a] = self.child_value(root, int(a))
        return self.root_proof, q


class ProveGuidedTree(TacticsGuidedTree, _Prove):
    """The plain restatement with proven values (no reroot: a plain session of the harness is a wide one of width 1)."""

    def __init__(self, game, root, simulations, depth):
        TacticsGuidedTree.__init__(self, game, root, simulations, depth)
        self.prove_init()
        self.done = 0

    def advance(self, priors, value):
        self.answered(self.status, self.pending, self.path)
        assert self.t <= self.S
        t, self.t = self.t, self.t + 1
        if self.status == 2:
            return
        leaf = self.nodes[self.pending]
        if self.status == 0:
            leaf["p"] = [clean(x) for x in priors]
            val0 = F(self.sign(leaf)) * cleanv(value)
        else:
            val0 = F(leaf["term0"])
        for n, a in self.path:
            self.nodes[n]["v"][a] += 1
            self.nodes[n]["w0"][a] = F(self.nodes[n]["w0"][a] + val0)
        self.done += bool(self.path)
        if self.status == 1:
            self.climb(self.path, self.pending)
        if t == self.S or self.root_proof != UNPROVEN:  # rule 5
            self.status = 2
            return
        node, self.path = 0, []
        while True:
            nd = self.nodes[node]
            total, sign = sum(nd["v"]), self.sign(nd)
            a = self.pick(nd, lambda b: score(nd["v"][b], nd["w0"][b], nd["p"][b], total, sign, self.c))
            self.path.append((node, a))
            if nd["child"][a] < 0:
                pos, term0 = self.expand(nd["pos"], a)
                node = nd["child"][a] = self._make(pos, term0)
                break
            node = nd["child"][a]
            if self.nodes[node]["pos"].done:
                break
        self.pending = node
        self.status = self.look_at(1 if self.nodes[node]["pos"].done else 0, node)

    def result(self):
        return self.prove_result(TacticsGuidedTree.result(self))


class ProveWideTree(TacticsWideTree, _Prove):
    """The wide restatement with proven values."""

    def __init__(self, game, root, simulations, width, depth, capacity=0):
        TacticsWideTree.__init__(self, game, root, simulations, width, depth, capacity)
        self.prove_init()

    def advance(self, priors, values):
        for s in self.slots:
            self.answered(s["status"], s["pending"], s["path"])
        assert self.t <= self.S
        self.t += 1
        # A. the answers, each status-1 slot's climb right behind its backup
        for j, s in enumerate(self.slots):
            if s["status"] == 2:
                continue
            leaf = self.nodes[s["pending"]]
            if s["status"] == 0:
                leaf["p"] = [clean(x) for x in priors[j]]
                val0 = F(self.sign(leaf)) * cleanv(values[j])
            else:
                val0 = F(leaf["term0"])
            for n, a in s["path"]:
                self.nodes[n]["v"][a] += 1
                self.nodes[n]["w0"][a] = F(self.nodes[n]["w0"][a] + val0)
            self.done += bool(s["path"])
            if s["status"] == 1:
                self.climb(s["path"], s["pending"])
            s["status"], s["path"] = 2, []
        if self.over or self.root_proof != UNPROVEN:  # rule 5
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
                total, sign = sum(nd["v"]) + sum(o), self.sign(nd)
                a = self.pick(nd, lambda b: wscore(nd["v"][b], nd["w0"][b], nd["p"][b], o[b], total, sign, self.c))
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
        for s in self.slots:  # the tactics stage, after ALL descents of the launch
            if s["status"] != 2:
                s["status"] = self.look_at(s["status"], s["pending"])

    def result(self):
        return self.prove_result(TacticsWideTree.result(self))

    def marked_below(self, c):
        """whether the subtree of node c holds a marked node other than c"""
        stack = [ch for ch in self.nodes[c]["child"] if ch >= 0]
        while stack:
            k = stack.pop()
            if self.nodes[k].get("marked"):
                return True
            stack.extend(ch for ch in self.nodes[k]["child"] if ch >= 0)
        return False

    def reroot_choice(self, want, fallback):
        """An action for reroot: `want` = "onto" a marked child, "deeper": a child with marked nodes below it; the
        fallback if there is none (or the root is over)."""
        if self.over:
            return max(fallback, 0)
        root = self.nodes[0]
        for a in np.flatnonzero(root["pos"].mask):
            c = root["child"][a]
            if c < 0:
                continue
            marked = bool(self.nodes[c].get("marked"))
            if (want == "onto" and marked) or (want == "deeper" and self.marked_below(c)):
                return int(a)
        return max(fallback, 0)

    def reroot(self, a, s2):
        """rule 8"""
        c = -1 if self.over else self.nodes[0]["child"][a]
        onto = c >= 0 and bool(self.nodes[c].get("marked"))
        if onto:
            self.nodes[c]["marked"] = False
        TacticsWideTree.reroot(self, a, s2)
        self.root_proof = UNPROVEN
        if not self.over and c >= 0:
            self.root_proof = self.rule2(self.nodes[0])
            assert not onto or self.root_proof != UNPROVEN  # a marked node's proof came from its kept children
        self.seen["onto"] += onto
        self.seen["deeper"] += any(nd.get("marked") for nd in self.nodes[1:])
        self.seen["at_once"] += self.root_proof != UNPROVEN


# ---- the harness's session ------------------------------------------------------------------------------------------
class ProveHost(TacticsHost):
    """TacticsHost begun through pgx_prove_begin with a flags word."""

    def __init__(self, libs, fam, poss, simulations, width, tactics, flags=PROVE, tactics_nodes=BIG, nodes=0,
                 want_rc=0):
        self.lib, self.n, self.n_act, self.W = libs["tactics"], len(poss), ACTIONS[fam], width
        hid = np.ascontiguousarray(np.stack([p.key[1] for p in poss]), np.int32)
        done = np.array([p.done for p in poss], np.uint8)
        self.obs = np.full((self.n, width) + SHAPE[fam], 7, np.uint8)
        self.mask = np.full((self.n, width, self.n_act), 7, np.uint8)
        self.status = np.full((self.n, width), 7, np.uint8)
        rc = ctypes.c_int(-9)
        self.h = self.lib.pgx_prove_begin(CODE[fam], self.n, _ptr(hid), _ptr(done), simulations,
                                          nodes or simulations + 1, width, ctypes.c_float(C_PUCT), int(tactics),
                                          ctypes.c_longlong(int(tactics_nodes)), int(flags), _ptr(self.obs),
                                          _ptr(self.mask), _ptr(self.status), ctypes.byref(rc))
        assert rc.value == want_rc and bool(self.h) == (want_rc == 0)
        self.tactics = True

    def proof(self):
        value, q = np.full(self.n, 7, np.int8), np.full((self.n, self.n_act), 7, np.int8)
        self.lib.pgx_prove_proof(ctypes.c_void_p(self.h), _ptr(value), _ptr(q))
        return value, q


class ProvePair(Pair):
    """Pair with proven values on both sides; `proof` is compared with everything else, call for call."""

    def __init__(self, libs, game, roots, simulations, width, depth, evaluator, nodes=0, wide_tree=None):
        self.game, self.roots, self.S, self.W, self.D = game, roots, simulations, width, depth
        self.fed = tu.EVALUATORS[evaluator]
        self.constant = evaluator == "constant"
        self.host = ProveHost(libs, game.fam, roots, simulations, width, depth, PROVE, BIG, nodes)
        self.wide_tree = (width > 1 or nodes != 0) if wide_tree is None else wide_tree
        if self.wide_tree:
            self.trees = [ProveWideTree(game, r, simulations, width, depth, nodes or simulations + 1) for r in roots]
        else:
            self.trees = [ProveGuidedTree(game, r, simulations, depth) for r in roots]
        self.calls = 0

    def same_result(self, what):
        got = Pair.same_result(self, what)
        value, q = self.host.proof()
        for i, tree in enumerate(self.trees):
            want = tree.proof()
            assert value[i] == want[0], (self.game.fam, what, i, value[i], want[0])
            assert np.array_equal(q[i], want[1]), (self.game.fam, what, i, q[i], want[1])
        return got

    def seen(self):
        out = dict.fromkeys(EVENTS, 0)
        for tree in self.trees:
            for k, v in tree.seen.items():
                out[k] += v
            out["result"] += bool(getattr(tree, "differs", False))
        return out


# ---- the roots and their truth --------------------------------------------------------------------------------------
def hex_late_roots(game):
    """Hex positions the brute force solves to the end: row y = 5 of color 0 (which joins x = 0 to x = 10; cell (x, y)
    is x * 11 + y) with holes, every other cell color 1 but for a few that matter to nobody.  Color 1 needs one hole of
    the row, color 0 all of them.  (No positions of a real game, but positions of the rules'.)"""
    def make(holes, spare, color0_moves):
        row = [x * 11 + 5 for x in range(11) if x not in holes]
        empty = {x * 11 + 5 for x in holes} | set(spare)
        rest = [c for c in range(121) if c not in row and c not in empty]
        stones = len(row) + len(rest)
        assert (stones % 2 == 0) == color0_moves  # even: color 0 is to move
        turn = stones
        if color0_moves:
            return game.pos(_hex_words(row, rest, turn, 0))
        return game.pos(_hex_words(rest, row, turn, 0))
    return [make((5,), (0, 120), True),        # color 0 wins at once, or dawdles and loses
            make((5,), (0, 120, 3), False),    # color 1 wins at once
            make((3, 7), (1,), True),          # color 0 needs two moves, color 1 one: lost
            make((3, 7), (1, 119), False),     # color 1 wins at once
            make((2, 5, 8), (), True),
            # four more, found by trying random holes and spare cells: the stand-in evaluator's search proves an
            # interior node lost in each (all its moves lead to positions proven won for the other side)
            make((0, 6), (56, 98), False),
            make((3, 5), (30, 81, 107), True),
            make((0, 1, 9), (45, 52), True),
            make((1, 10), (114,), True)]


def late_roots(libs, game, n, plies, seed):
    """n roots exactly `plies` seeded random legal plies from the reset: roll-outs that end earlier are thrown away, so
    every root is as late as asked and the brute force finishes it."""
    hid, _ = host_reset(libs["host"], game.fam, 1, 11)
    out = []
    while len(out) < n:
        rng = np.random.default_rng(seed)
        seed += 1
        pos = game.pos(hid[0])
        for _ in range(plies):
            pos, _ = game.expand(pos, int(rng.choice(np.flatnonzero(pos.mask))))
            if pos.done:
                break
        if not pos.done:
            out.append(pos)
        assert seed < 100000
    return out


def root_set(libs, game):
    """The roots of one game's tests: late rolled or hand-made ones, one that is over at begin, one with a single legal
    move."""
    fam = game.fam
    if fam == "Hex":
        roots = hex_late_roots(game)
    else:
        lo, hi = PLIES[fam]
        roots = []
        for j, plies in enumerate(range(lo, hi + 1)):
            roots += late_roots(libs, game, ROLLED, plies, ROLL_SEED[fam] + 1000 * j)
        if fam == "Othello":  # draws are rare: two roots 57 plies in whose exact value is 0 (by the brute force)
            for seed in OTHELLO_DRAWS:
                roots += late_roots(libs, game, 1, 57, seed)
    return roots + [over_root(game, roots[0]), single_move_root(libs, game)]


def truth(libs, game, roots):
    """The brute force's full solve (depth 0) of every running root: (value int8 [n], q int8 [n, A]); None for a root
    that is over."""
    out = []
    for r in roots:
        if r.done:
            out.append(None)
            continue
        (value, q, _, status), _ = brute_solve(libs["brute"], game.fam, r.key[1][None], [0], 0)
        assert status[0] == 0
        out.append((int(value[0]), np.asarray(q[0], np.int8)))
    return out
