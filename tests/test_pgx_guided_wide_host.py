"""PGX guided search, several leaves per launch, CPU side: the wide sessions of envpool_amd/csrc/pgx_guided.hip.h built
for the host by g++ (tests/cpu_harness/pgx_guided_wide_host.cpp walks a wave's lanes as loops) against the contract
restated in numpy (pgx_guided_wide_util.py), both fed the stand-in evaluator, compared after every call bit for bit;
width 1 against the plain harness and the plain restatement; the consequences the header lists; and the argument checks
of the Python layers, which come before any native call."""
import ctypes

import numpy as np
import pytest

import test_pgx_guided_host as base
from pgx_guided_util import GuidedTree, stand_in
from pgx_guided_wide_util import WideTree, wscore
from pgx_guided_util import score
from pgx_util import ACTIONS, CODE, game

GAMES = base.GAMES
F = np.float32


def sims(tid):
    return 12 if tid.startswith("Hex") else 24


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pgx_guided_wide")
    wide = base._build(tmp, "pgx_guided_wide_host.cpp", "libpgxwidehost.so")
    wide.pgx_wide_begin.restype = ctypes.c_void_p
    wide.pgx_wide_result.restype = None
    wide.pgx_wide_end.restype = None
    guided = base._build(tmp, "pgx_guided_host.cpp", "libpgxguidedhost.so")
    guided.pgx_guided_begin.restype = ctypes.c_void_p
    guided.pgx_guided_result.restype = None
    guided.pgx_guided_end.restype = None
    return base._build(tmp, "pgx_host.cpp", "libpgxhost.so"), guided, wide


_ptr = base._ptr


class WideSession:
    """The harness's wide session over the roots `poss`; leaf arrays [n, W, ...]."""

    def __init__(self, libs, tid, poss, simulations, c_puct, width, nodes=0, want_rc=0):
        self.lib, self.n, self.n_act, self.W = libs[2], len(poss), ACTIONS[game(tid)], width
        hid = np.ascontiguousarray(np.stack([p.key[1] for p in poss]), np.int32)
        done = np.array([p.done for p in poss], np.uint8)
        w = max(width, 1)
        self.obs = np.full((self.n, w) + poss[0].obs.shape, 7, np.uint8)
        self.mask = np.full((self.n, w, self.n_act), 7, np.uint8)
        self.status = np.full((self.n, w), 7, np.uint8)
        rc = ctypes.c_int(-9)
        self.h = self.lib.pgx_wide_begin(CODE[game(tid)], self.n, _ptr(hid), _ptr(done), simulations,
                                         nodes or simulations + 1, width, ctypes.c_float(c_puct), _ptr(self.obs),
                                         _ptr(self.mask), _ptr(self.status), ctypes.byref(rc))
        assert rc.value == want_rc and bool(self.h) == (want_rc == 0)

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

    def reroot(self, actions, s2):
        actions = np.ascontiguousarray(actions, np.int32)
        return self.lib.pgx_wide_reroot(ctypes.c_void_p(self.h), _ptr(actions), s2, _ptr(self.obs), _ptr(self.mask),
                                        _ptr(self.status))

    def close(self):
        self.lib.pgx_wide_end(ctypes.c_void_p(self.h))
        self.h = None


def evaluate(obs, mask):
    """stand_in over leaf arrays with the slot axis: ([n, W, A], [n, W])."""
    n, w = mask.shape[:2]
    priors, values = stand_in(obs.reshape((n * w,) + obs.shape[2:]), mask.reshape(n * w, -1))
    return priors.reshape(n, w, -1), values.reshape(n, w)


class Pair:
    """The numpy restatement and the harness from one position, fed the same numbers and compared after every call."""

    def __init__(self, libs, game_, pos, simulations, c_puct, width, nodes=0):
        self.game, self.pos, self.S, self.W, self.C = game_, pos, simulations, width, nodes or simulations + 1
        self.tree = WideTree(pos, pos.done, game_.expand, simulations, c_puct, width, self.C)
        self.host = WideSession(libs, game_.tid, [pos], simulations, c_puct, width, nodes)
        self.kept = 0  # the root's visits at the round's start (after a reroot)
        self.advances = []

    def same_leaves(self, t):
        obs, mask, status = self.host.leaves()
        want = self.tree.leaves()
        assert np.array_equal(status[0], want[2]), (self.game.tid, t, status[0], want[2])
        assert np.array_equal(obs[0].astype(bool), want[0]) and np.array_equal(mask[0].astype(bool), want[1]), t
        assert set(np.unique(obs)) <= {0, 1} and set(np.unique(mask)) <= {0, 1}
        idle = status[0] != 0
        assert not obs[0][idle].any() and not mask[0][idle].any()
        return obs, mask, status

    def same_result(self, t):
        got, ref = self.host.result(), self.tree.result()
        assert np.array_equal(got[0][0], ref[0]), (self.game.tid, t, got[0][0], ref[0])
        assert np.array_equal(base.bits(got[1][0]), base.bits(ref[1])), (self.game.tid, t, got[1][0], ref[1])
        assert got[2][0] == ref[2] and got[3][0] == ref[3] and got[4][0] == ref[4], (t, got[2:], ref[2:])
        return got

    def round(self, spoil=None, fed=evaluate):
        """Advances until the round is complete, checking the header's consequences on the way.  Returns the result
        and the statuses seen per call."""
        seen, t = [], 0
        while True:
            obs, mask, status = self.same_leaves(t)
            seen.append(status[0].tolist())
            if (status == 2).all():
                break
            assert t <= self.S, "a round is complete after at most S + 1 advances"
            live = [self.tree.slots[j]["pending"] for j in range(self.W) if status[0][j] == 0]
            assert len(live) == len(set(live))  # no two status-0 slots share a node
            priors, values = fed(obs, mask)
            if spoil is not None:
                spoil(t, priors, values, status)
            before = self.host.result()
            assert self.host.advance(priors, values) == 0
            self.tree.advance(priors[0], values[0])
            got = self.same_result(t)
            pending = int((status[0] != 2).sum()) - (1 if t == 0 and not self.pos.done else 0)
            assert got[4][0] == before[4][0] + pending  # every answered descent is a simulation
            assert got[0].sum() == self.kept + got[4][0] and got[4][0] <= self.S
            assert got[3][0] <= self.C
            if before[4][0] < self.S and before[3][0] < self.C and t > 0:
                assert got[4][0] > before[4][0]  # slot 0 never collides: every advance completes a simulation
            t += 1
        self.advances.append(t)
        # later advances on a complete round change nothing; a call number above S is refused
        final = self.host.result()
        zeros = np.zeros((1, self.W, self.tree.n_act), F), np.zeros((1, self.W), F)
        for _ in range(t, self.S + 1):
            assert self.host.advance(*zeros) == 0
            assert (self.host.status == 2).all() and not self.host.obs.any() and not self.host.mask.any()
        for x, y in zip(final, self.host.result()):
            assert np.array_equal(x, y)
        assert self.host.advance(*zeros) == -4
        return final, seen

    def reroot(self, a, s2=None):
        s2 = s2 or self.S
        assert self.host.reroot([a], s2) == 0
        self.tree.reroot(a, s2)
        self.S = s2
        self.kept = int(self.host.result()[0].sum())
        self.same_leaves("reroot")
        self.same_result("reroot")

    def close(self):
        self.host.close()


def start(libs, tid, mid=True):
    game_ = base.Replayed(libs, tid, column=2 if mid else 1)
    return game_, game_.fixture_row(base.mid_row(game_.g, 2) if mid else 0)


# ---- the score ------------------------------------------------------------------------------------------------------
def test_wscore_without_virtual_losses_is_score_bit_for_bit():
    rng = np.random.default_rng(3)
    for _ in range(2000):
        v, total = int(rng.integers(0, 50)), int(rng.integers(0, 500))
        w0, p, c = F(rng.normal() * v), F(rng.random()), F(rng.choice([0.0, 1.25, 3.0]))
        if rng.random() < 0.1:
            w0 = F(-0.0)
        sign = int(rng.choice([-1, 1]))
        assert wscore(v, w0, p, 0, total, sign, c).view(np.uint32) == score(v, w0, p, total, sign, c).view(np.uint32)
    # a virtual loss lowers an edge's score: one more visit that lost, and a smaller exploration term
    assert wscore(3, F(1.5), F(0.2), 1, 10, 1, 1.25) < wscore(3, F(1.5), F(0.2), 0, 9, 1, 1.25)
    assert wscore(0, F(0.0), F(0.2), 2, 10, 1, 0.0) == F(-1.0)


# ---- harness == restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [2, 4, 8])
@pytest.mark.parametrize("tid", GAMES)
def test_wide_session_equals_the_numpy_restatement(libs, tid, width):
    S = sims(tid)
    game_, pos = start(libs, tid)
    pair = Pair(libs, game_, pos, S, 1.25, width)
    (visits, values, action, nodes, done), seen = pair.round()
    pair.close()
    assert visits.sum() == S and done[0] == S and nodes[0] == len(game_.expanded) + 1 <= S + 1
    assert action[0] >= 0 and pos.mask[action[0]]
    assert (visits[0][~pos.mask] == 0).all() and (values[0][~pos.mask] == 0).all()
    assert seen[0] == [0] + [2] * (width - 1)  # the root's own evaluation: slot 0 alone
    assert pair.advances[0] <= S + 1
    if pos.mask.sum() >= width:
        assert pair.advances[0] < S + 1  # fewer model calls than the plain session's S + 1
        assert max(sum(st != 2 for st in row) for row in seen) == width  # a launch that handed out W leaves


@pytest.mark.parametrize("tid", GAMES)
def test_width_1_is_the_plain_session_call_for_call(libs, tid):
    S = sims(tid)
    game_, pos = start(libs, tid)
    over = game_.fixture_row(int(np.flatnonzero(game_.g["done"][:, 2])[0]))
    poss = [pos, over, game_.fixture_row(0)]
    wide = WideSession(libs, tid, poss, S, 1.25, 1)
    plain = base.HostSession((libs[0], libs[1]), tid, poss, S, 1.25)
    trees = [GuidedTree(p, p.done, base.Replayed(libs, tid, column=2).expand, S, 1.25) for p in poss]
    for t in range(S + 1):
        got, ref = wide.leaves(), plain.leaves()
        assert np.array_equal(got[0][:, 0], ref[0]) and np.array_equal(got[1][:, 0], ref[1]), (tid, t)
        assert np.array_equal(got[2][:, 0], ref[2]), (tid, t, got[2], ref[2])
        priors, values = stand_in(ref[0], ref[1])
        assert wide.advance(priors[:, None], values[:, None]) == 0 and plain.advance(priors, values) == 0
        w, p = wide.result(), plain.result()
        for x, y in zip(w[:4], p):
            assert np.array_equal(x, y), (tid, t)
        for i, tree in enumerate(trees):
            tree.advance(priors[i], values[i])
            r = tree.result()
            assert np.array_equal(w[0][i], r[0]) and np.array_equal(base.bits(w[1][i]), base.bits(r[1]))
            assert w[2][i] == r[2] and w[3][i] == r[3]
    assert (wide.status == 2).all() and wide.advance(priors[:, None], values[:, None]) == -4
    assert wide.result()[4].tolist() == [S, 0, S]
    wide.close()
    plain.close()


@pytest.mark.parametrize("S,width", [(10, 4), (7, 8), (5, 3), (1, 4)])
def test_simulations_that_are_no_multiple_of_the_width(libs, S, width):
    game_, pos = start(libs, "ConnectFour-v1")
    pair = Pair(libs, game_, pos, S, 1.25, width)
    (visits, _, _, _, done), seen = pair.round()
    pair.close()
    assert visits.sum() == S == done[0]
    handed = [sum(st != 2 for st in row) for row in seen[1:-1]]
    assert sum(handed) == S and all(1 <= h <= width for h in handed)  # never more descents than simulations left


def test_capacity_reached_in_mid_launch(libs):
    """A rerooted tree keeps its nodes, so S2 more simulations do not fit into C: the launch that reaches C stops handing
    out leaves, the later ones hand out none, and no error is set."""
    S, C, W = 24, 30, 4
    game_, pos = start(libs, "Othello-v1")
    pair = Pair(libs, game_, pos, S, 1.25, W, nodes=C)
    (visits, _, action, nodes, _), _ = pair.round()
    pair.reroot(int(action[0]))
    kept_nodes = int(pair.host.result()[3][0])
    assert kept_nodes > 3 and C - kept_nodes < S and (C - kept_nodes) % W != 0  # C is met inside a launch
    (visits2, _, _, nodes2, done2), seen = pair.round()
    pair.close()
    assert nodes2[0] == C and done2[0] < S and visits2.sum() == pair.kept + done2[0]
    handed = [sum(st != 2 for st in row) for row in seen]
    assert any(0 < h < W for h in handed[1:-1])


def forced_pass(libs):
    """An Othello position whose only legal move is the pass."""
    game_ = base.Replayed(libs, "Othello-v1", column=0)
    rng = np.random.default_rng(5)
    for _ in range(400):
        seq = []
        pos, _ = game_.at(seq)
        while not pos.done:
            if pos.mask[64]:
                assert pos.mask.sum() == 1
                return game_, pos
            seq.append(int(rng.choice(np.flatnonzero(pos.mask))))
            pos, _ = game_.at(seq)
    raise AssertionError("no forced pass found")


def test_a_forced_collision_leaves_the_other_slots_idle(libs):
    """A root with a single legal move: descent 1 of the first launch arrives at the node that descent 0 just made, a
    collision -- slots 1.. stay idle -- and the round still completes within S + 1 advances."""
    S, W = 24, 4
    game_, pos = forced_pass(libs)
    pair = Pair(libs, game_, pos, S, 1.25, W)
    (visits, _, action, _, done), seen = pair.round()
    pair.close()
    assert seen[0] == [0, 2, 2, 2] and seen[1] == [0, 2, 2, 2]
    assert pair.tree.collisions >= 1 and pair.advances[0] <= S + 1
    assert action[0] == 64 and visits[0][64] == S == done[0]


def test_two_slots_on_one_finished_game(libs):
    """TicTacToe with one empty cell: the only move ends the game, so every slot of a launch reaches the same finished
    node: all have status 1, all back up term0, and that is no collision."""
    S, W = 10, 4
    game_ = base.Replayed(libs, "TicTacToe-v1", column=0)
    pos, _ = game_.at([0, 1, 2, 4, 3, 5, 7, 6])
    assert not pos.done and pos.mask.sum() == 1 and pos.mask[8]

    def spoil(t, priors, values, status):  # whatever the caller says in a row of status 1 is ignored
        priors[0][status[0] == 1] = 1e30
        values[0][status[0] == 1] = 1.0 if t % 2 else -1.0

    pair = Pair(libs, game_, pos, S, 1.25, W)
    (visits, values, action, nodes, done), seen = pair.round(spoil=spoil)
    pair.close()
    assert seen[:5] == [[0, 2, 2, 2], [1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 2, 2], [2, 2, 2, 2]]
    term = game_.at([0, 1, 2, 4, 3, 5, 7, 6, 8])[1]
    mover_sign = 1 if pos.mover == 0 else -1
    assert nodes[0] == 2 and visits[0][8] == S and values[0][8] == F(S * mover_sign * term[0]) and action[0] == 8
    assert pair.tree.collisions == 0


def test_width_32_on_tictactoe_has_more_slots_than_moves(libs):
    S = 40
    game_ = base.Replayed(libs, "TicTacToe-v1", column=1)
    pos = game_.fixture_row(0)
    pair = Pair(libs, game_, pos, S, 1.25, 32)
    (visits, _, _, nodes, done), seen = pair.round()
    pair.close()
    assert visits.sum() == S == done[0] and pair.advances[0] < S // 2
    assert max(sum(st != 2 for st in row) for row in seen) > 9  # virtual losses spread a launch below the root


def test_rows_are_cleaned_per_slot(libs):
    """clean / cleanv act on the row of the slot they belong to: spoiled entries in some slots equal zeros there, and the
    other slots' rows are used as given."""
    S, W = 24, 4
    bad = [np.nan, -1.0, np.inf, -np.inf, -1e-30, 3.5e38]

    def spoil(zero):
        def fn(t, priors, values, status):
            for j in range(W):
                if status[0][j] == 0 and (t + j) % 2 == 0:
                    legal = np.flatnonzero(priors[0][j] > 0)[: len(bad)]
                    priors[0][j][legal] = 0.0 if zero else np.array(bad[: len(legal)], F)
                    values[0][j] = 0.0 if zero else [np.nan, 1.5, -2.0, np.inf][(t + j) % 4]
        return fn

    results = []
    for zero in (False, True):
        game_, pos = start(libs, "Othello-v1")
        pair = Pair(libs, game_, pos, S, 1.25, W)
        with np.errstate(over="ignore", invalid="ignore"):
            results.append(pair.round(spoil=spoil(zero)))
        pair.close()
    for x, y in zip(results[0][0], results[1][0]):
        assert np.array_equal(x, y)
    assert results[0][1] == results[1][1]
    game_, pos = start(libs, "Othello-v1")
    plain = Pair(libs, game_, pos, S, 1.25, W)
    assert not np.array_equal(plain.round()[0][0], results[0][0][0])  # the spoiled entries mattered
    plain.close()


# ---- reroot ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tid", GAMES)
def test_three_moves_of_a_wide_session_with_reroot(libs, tid):
    S, W = sims(tid), 4
    game_, pos = start(libs, tid, mid=not tid.startswith("TicTacToe"))  # (three more moves have to fit)
    pair = Pair(libs, game_, pos, S, 1.25, W, nodes=3 * S + 1)
    total = 0
    for move in range(3):
        (visits, _, action, nodes, done), seen = pair.round()
        if action[0] < 0:
            break
        assert visits.sum() == pair.kept + pair.S and done[0] == pair.S  # the kept visits add to the round's S2
        total += 1
        pair.reroot(int(action[0]), S if move == 0 else S - 3)
        assert pair.host.status[0].tolist() in ([0] + [2] * (W - 1), [2] * W) and pair.host.result()[4][0] == 0
    pair.close()
    assert total >= 2


@pytest.mark.parametrize("tid", ["TicTacToe-v1", "Hex-v1"])
def test_width_16(libs, tid):
    """The width of the kernel's middle path bucket (5 .. 16 slots)."""
    S = sims(tid)
    game_, pos = start(libs, tid)
    pair = Pair(libs, game_, pos, S, 1.25, 16)
    (visits, _, action, nodes, done), seen = pair.round()
    pair.close()
    assert visits.sum() == S == done[0] and nodes[0] <= S + 1 and pos.mask[action[0]]
    assert seen[0] == [0] + [2] * 15 and pair.advances[0] < S + 1
    if pos.mask.sum() >= 16:
        assert max(sum(st != 2 for st in row) for row in seen) > 4  # more leaves in a launch than the first bucket holds


@pytest.mark.parametrize("tid,nodes", [("ConnectFour-v1", 513), ("ConnectFour-v1", 2049), ("ConnectFour-v1", 8192),
                                       ("Hex-v1", 513), ("Hex-v1", 2049)])
def test_wide_reroot_at_capacities_above_512_and_2048_nodes(libs, tid, nodes):
    """The capacities of the reroot kernel's two larger tables: a round of 8 simulations, a reroot by the chosen move,
    a second round."""
    S, W = 8, 4
    game_, pos = start(libs, tid)
    pair = Pair(libs, game_, pos, S, 1.25, W, nodes=nodes)
    (visits, _, action, _, done), _ = pair.round()
    a = int(action[0])
    assert done[0] == S and visits[0][a] >= 1  # the most visited move has a child: the table path runs
    pair.reroot(a)
    if pair.host.status[0][0] == 0:  # (else the move ended the game)
        assert pair.kept == visits[0][a] - 1 and 1 <= pair.host.result()[3][0] <= visits[0][a]
        (after, _, _, used, done), _ = pair.round()
        assert after.sum() == pair.kept + S and done[0] == S and used[0] <= nodes
    pair.close()


def test_reroot_with_pending_slots(libs):
    """The host forms refuse a reroot while a slot is pending; the device form cannot look: the pending slots are dropped,
    nothing of them is backed up, and their nodes stay unevaluated."""
    S, W = 24, 4
    game_, pos = start(libs, "ConnectFour-v1")
    pair = Pair(libs, game_, pos, S, 1.25, W, nodes=2 * S + 1)
    for t in range(3):
        obs, mask, status = pair.same_leaves(t)
        assert pair.host.reroot([3], S) == -5
        priors, values = evaluate(obs, mask)
        assert pair.host.advance(priors, values) == 0
        pair.tree.advance(priors[0], values[0])
    assert (pair.host.status[0] != 2).sum() == W
    before = pair.host.result()
    a = int(np.argmax(before[0][0]))
    assert pair.host.reroot([a], -S) == 0  # (the harness's stand-in for the device form)
    pair.tree.reroot(a, S)
    pair.kept = int(pair.host.result()[0].sum())
    pair.same_leaves("reroot")
    pair.same_result("reroot")
    assert pair.host.status[0].tolist() == [0, 2, 2, 2]
    (visits, _, _, _, done), _ = pair.round()
    assert done[0] == S and visits.sum() == pair.kept + S
    pair.close()


def test_roots_that_are_over_and_several_roots(libs):
    game_, pos = start(libs, "TicTacToe-v1")
    over = game_.fixture_row(int(np.flatnonzero(game_.g["done"][:, 2])[0]))
    assert over.done
    W, S = 4, 12
    host = WideSession(libs, "TicTacToe-v1", [over, pos, over], S, 1.25, W)
    single = Pair(libs, game_, pos, S, 1.25, W)
    for t in range(S + 1):
        obs, mask, status = host.leaves()
        assert (status[[0, 2]] == 2).all() and not obs[[0, 2]].any() and not mask[[0, 2]].any()
        one = single.host.leaves()
        for x, y in zip((obs, mask, status), one):
            assert np.array_equal(x[1], y[0]), t
        priors, values = evaluate(obs, mask)
        assert host.advance(priors, values) == 0 and single.host.advance(priors[1:2], values[1:2]) == 0
    got, ref = host.result(), single.host.result()
    for x, y in zip(got, ref):
        assert np.array_equal(x[1], y[0])
    assert got[2].tolist()[::2] == [-1, -1] and not got[0][[0, 2]].any() and not got[1][[0, 2]].any()
    assert host.reroot([0, int(got[2][1]), 0], S) == 0 and (host.status[[0, 2]] == 2).all()
    host.close()
    single.close()


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_harness_refusals(libs):
    pos = base.Replayed(libs, "ConnectFour-v1", column=1).fixture_row(0)
    for S, nodes, width in ((4, 5, 0), (4, 5, 33), (4, 5, -1), (4, 4, 4), (0, 5, 4), (4, 8193, 4)):
        WideSession(libs, "ConnectFour-v1", [pos], S, 1.25, width, nodes, want_rc=-6)
    host = WideSession(libs, "ConnectFour-v1", [pos], 4, 1.25, 32, 8)
    assert host.reroot([3], 4) == -5  # the root itself is pending
    host.close()
    assert libs[2].pgx_wide_root_bytes(1) % 16 == 0 and libs[2].pgx_wide_root_bytes(32) < 40 * 1024


def test_check_guided_width_and_wide_rows():
    from envpool_amd.core import native

    assert native.GUIDED_MAX_WIDTH == 32
    assert native.check_guided_width(None) == 0 and native.check_guided_width(1) == 1
    assert native.check_guided_width(32) == 32 and native.check_guided_width(np.int64(8)) == 8
    for width in (0, 33, -1, 2.5, True):
        with pytest.raises(ValueError, match="guided_begin: width"):
            native.check_guided_width(width)
    priors, values = np.full((3, 4, 9), 0.25, np.float64), np.zeros((3, 4))
    p, v = native.check_guided_wide_rows(priors, values, 3, 4, 9)
    assert p.shape == (12, 9) and v.shape == (12,) and p.dtype == v.dtype == np.float32 and p.flags.c_contiguous
    p, v = native.check_guided_wide_rows(priors.reshape(12, 9), values.reshape(12), 3, 4, 9)
    assert p.shape == (12, 9) and v.shape == (12,)
    for bad_p, bad_v in ((priors[:2], values), (priors, values[:, :3]), (priors.reshape(4, 3, 9), values),
                         (priors.reshape(3, 36), values), (priors, values.reshape(4, 3))):
        with pytest.raises(ValueError, match="guided_advance"):
            native.check_guided_wide_rows(bad_p, bad_v, 3, 4, 9)
    spoiled = priors.copy()
    spoiled[2, 3, 8] = np.nan
    with pytest.raises(ValueError, match="priors must be finite"):
        native.check_guided_wide_rows(spoiled, values, 3, 4, 9)
    with pytest.raises(ValueError, match="values must be in"):
        native.check_guided_wide_rows(priors, values + 1.5, 3, 4, 9)


class _Recorder(base._Recorder):
    """A pool that records the guided calls it gets; with a width its leaves carry the slot axis, and a round is over
    after `rounds` advances."""

    rounds = 3

    def guided_begin(self, env_ids, simulations, c_puct, nodes=None, width=None):
        out = super().guided_begin(env_ids, simulations, c_puct)
        if nodes is not None or width is not None:
            self.calls[-1] += (nodes, width)
        self.width, self.made = width, 0
        return self._leaves()

    def _leaves(self):
        if not getattr(self, "width", None):
            return super()._leaves()
        status = np.full((self.k, self.width), 2 if self.made >= self.rounds else 0, np.uint8)
        return np.zeros((self.k, self.width, 8, 8, 2), bool), np.zeros((self.k, self.width, 65), bool), status

    def guided_advance(self, priors, values):
        self.made += 1
        return super().guided_advance(priors, values)

    def guided_reroot(self, actions, simulations):
        self.calls.append(("reroot", np.asarray(actions).tolist(), simulations))
        self.made = 0
        return self._leaves()


def test_wrapper_checks_come_before_the_native_call():
    from envpool_amd.pgx import OthelloGymnasiumEnvPool

    env = object.__new__(OthelloGymnasiumEnvPool)
    env._pool = _Recorder()
    ids = np.array([2, 0, 1], np.int32)
    for width in (0, 33, -2, 1.5):
        with pytest.raises(ValueError, match="guided_begin: width"):
            env.guided_search(ids, simulations=8, width=width)
    with pytest.raises(ValueError, match="gumbel"):
        env.guided_search(ids, simulations=8, policy="gumbel", width=4)
    with pytest.raises(ValueError, match="gumbel_search: width"):
        env.gumbel_search(ids, simulations=8, width=4)
    assert env._pool.calls == []
    # the default is today's object and calls
    gs = env.guided_search(ids, simulations=3, c_puct=0.5)
    assert env._pool.calls == [("begin", [2, 0, 1], 3, 0.5)] and gs.width == 1 and not gs.done
    gs.close()
    gs = env.guided_search(ids, simulations=3, c_puct=0.5, width=1, nodes=9)
    assert env._pool.calls[-1] == ("begin", [2, 0, 1], 3, 0.5, 9, None)
    gs.close()
    env._pool.calls.clear()
    gs = env.guided_search(ids, simulations=8, c_puct=0.5, nodes=20, width=4)
    assert env._pool.calls == [("begin", [2, 0, 1], 8, 0.5, 20, 4)] and gs.width == 4
    assert gs.leaves[0].shape == (3, 4, 8, 8, 2) and gs.leaves[2].shape == (3, 4) and not gs.done
    shapes = []

    def model(obs, mask, status):  # a model function written for the plain session: flat rows
        shapes.append((obs.shape, mask.shape, status.shape))
        return np.zeros((len(obs), 65), np.float32), np.zeros(len(obs), np.float32)

    with pytest.raises(ValueError, match="round is not complete: 12 slots are pending"):
        gs.reroot([1, 2, 3])
    out = gs.run(model, close=False)
    assert out._fields == ("visits", "values", "action") and gs.done and gs.calls == 3
    assert shapes == [((12, 8, 8, 2), (12, 65), (12,))] * 3
    assert [c[0] for c in env._pool.calls] == ["begin"] + ["advance"] * 3 + ["result"]
    assert env._pool.calls[1] == ("advance", (12, 65), (12,))
    gs.reroot([1, 2, 3], simulations=5)
    assert env._pool.calls[-1] == ("reroot", [1, 2, 3], 5) and gs.calls == 0 and not gs.done
    gs.advance(np.zeros((3, 4, 65), np.float32), np.zeros((3, 4), np.float32))  # with the slot axis, too
    assert env._pool.calls[-1] == ("advance", (3, 4, 65), (3, 4))
    gs.run(model)
    assert [c[0] for c in env._pool.calls][-2:] == ["result", "end"]
    with pytest.raises(ValueError, match="closed"):
        gs.reroot([1, 2, 3])
