"""Tree reuse of the PGX guided search, CPU side: reroot of envpool_amd/csrc/pgx_guided.hip.h built for the host by g++
(tests/cpu_harness/pgx_reroot_host.cpp, a harness that walks a wave's lanes as loops and compacts the tree in place)
against the contract restated in numpy on a pointer tree (pgx_reroot_util.py), where reroot just takes the child.  Every
position, observation and expansion step comes from the reference-pinned `pgx_replay` of the PGX host harness; the
evaluator is the deterministic hash of pgx_guided_util.  And the argument checks of the Python wrappers, which come
before any native call."""
import ctypes

import numpy as np
import pytest

import test_pgx_guided_host as base
from pgx_guided_util import stand_in
from pgx_reroot_util import RerootTree
from pgx_util import ACTIONS, CODE, game

GAMES = base.GAMES
F = np.float32
_ptr = base._ptr
bits = base.bits


def sims(tid):
    return 12 if tid == "Hex-v1" else 24


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pgx_reroot")
    reroot = base._build(tmp, "pgx_reroot_host.cpp", "libpgxreroothost.so")
    reroot.pgx_reroot_begin.restype = ctypes.c_void_p
    reroot.pgx_reroot_result.restype = None
    reroot.pgx_reroot_end.restype = None
    guided = base._build(tmp, "pgx_guided_host.cpp", "libpgxguidedhost.so")
    guided.pgx_guided_begin.restype = ctypes.c_void_p
    guided.pgx_guided_result.restype = None
    guided.pgx_guided_end.restype = None
    return base._build(tmp, "pgx_host.cpp", "libpgxhost.so"), guided, reroot


class RerootSession:
    """The reroot harness's session over the roots `poss` (Pos with key = (seq, hidden words))."""

    def __init__(self, libs, tid, poss, simulations, c_puct, nodes, want_rc=0):
        self.lib, self.n, self.n_act = libs[2], len(poss), ACTIONS[game(tid)]
        hid = np.ascontiguousarray(np.stack([p.key[1] for p in poss]), np.int32)
        done = np.array([p.done for p in poss], np.uint8)
        self.obs = np.full((self.n,) + poss[0].obs.shape, 7, np.uint8)
        self.mask = np.full((self.n, self.n_act), 7, np.uint8)
        self.status = np.full(self.n, 7, np.uint8)
        rc = ctypes.c_int(-9)
        self.h = self.lib.pgx_reroot_begin(CODE[game(tid)], self.n, _ptr(hid), _ptr(done), simulations, nodes,
                                           ctypes.c_float(c_puct), _ptr(self.obs), _ptr(self.mask), _ptr(self.status),
                                           ctypes.byref(rc))
        assert rc.value == want_rc and bool(self.h) == (want_rc == 0)

    def leaves(self):
        return self.obs.copy(), self.mask.copy(), self.status.copy()

    def advance(self, priors, values):
        priors, values = np.ascontiguousarray(priors, F), np.ascontiguousarray(values, F)
        assert priors.shape == (self.n, self.n_act) and values.shape == (self.n,)
        return self.lib.pgx_reroot_advance(ctypes.c_void_p(self.h), _ptr(priors), _ptr(values), _ptr(self.obs),
                                           _ptr(self.mask), _ptr(self.status))

    def result(self):
        visits, values = np.full((self.n, self.n_act), -7, np.int32), np.full((self.n, self.n_act), -7, F)
        action, nodes = np.full(self.n, -7, np.int32), np.zeros(self.n, np.int32)
        self.lib.pgx_reroot_result(ctypes.c_void_p(self.h), _ptr(visits), _ptr(values), _ptr(action), _ptr(nodes))
        return visits, values, action, nodes

    def reroot(self, actions, simulations):
        actions = np.ascontiguousarray(actions, np.int32)
        assert actions.shape == (self.n,)
        return self.lib.pgx_reroot_reroot(ctypes.c_void_p(self.h), _ptr(actions), simulations, _ptr(self.obs),
                                          _ptr(self.mask), _ptr(self.status))

    def close(self):
        self.lib.pgx_reroot_end(ctypes.c_void_p(self.h))
        self.h = None


def same_result(got, ref, what):
    """row 0 of the harness's result against the restatement's, bit for bit"""
    assert np.array_equal(got[0][0], ref[0]), (what, got[0][0], ref[0])
    assert np.array_equal(bits(got[1][0]), bits(ref[1])), (what, got[1][0], ref[1])
    assert got[2][0] == ref[2] and got[3][0] == ref[3], (what, got[2][0], ref[2], got[3][0], ref[3])


class Pair:
    """The harness and the numpy restatement from one root, fed the same evaluator and compared after every call."""

    def __init__(self, libs, game_, pos, simulations, c_puct, nodes, evaluate=stand_in):
        self.game, self.evaluate, self.S = game_, evaluate, simulations
        self.tree = RerootTree(pos, pos.done, game_.expand, simulations, c_puct, nodes)
        self.host = RerootSession(libs, game_.tid, [pos], simulations, c_puct, nodes or simulations + 1)
        self.same_leaves("begin")

    def same_leaves(self, what):
        obs, mask, status = self.host.leaves()
        want = self.tree.leaf()
        assert status[0] == want[2], (self.game.tid, what, status[0], want[2])
        assert np.array_equal(obs[0].astype(bool), want[0]) and np.array_equal(mask[0].astype(bool), want[1]), what
        assert set(np.unique(obs)) <= {0, 1} and set(np.unique(mask)) <= {0, 1}
        if status[0] != 0:
            assert not obs.any() and not mask.any()
        return obs, mask, status

    def round(self):
        """simulations + 1 advances; returns the harness's result and the statuses handed out"""
        seen = []
        for t in range(self.S + 1):
            obs, mask, status = self.same_leaves(t)
            seen.append(int(status[0]))
            priors, values = self.evaluate(obs, mask)
            assert self.host.advance(priors, values) == 0  # (never an error, memory used up included)
            self.tree.advance(priors[0], values[0])
            same_result(self.host.result(), self.tree.result(), (self.game.tid, t))
        self.same_leaves("end")
        assert self.host.status[0] == 2
        assert self.host.advance(priors, values) == -4  # a call number above S
        return self.host.result(), seen

    def reroot(self, a, simulations=None):
        self.S = self.S if simulations is None else simulations
        assert self.host.reroot([a], self.S) == 0
        self.tree.reroot(a, self.S)
        leaves = self.same_leaves(("reroot", a))
        same_result(self.host.result(), self.tree.result(), ("reroot", a))
        return leaves

    def close(self):
        self.host.close()


def start(libs, tid, mid):
    game_ = base.Replayed(libs, tid, column=2 if mid else 1)
    pos = game_.fixture_row(base.mid_row(game_.g, 2) if mid else 0)
    assert not pos.done
    return game_, pos


@pytest.mark.parametrize("mid", [False, True])
@pytest.mark.parametrize("tid", GAMES)
def test_three_moves_with_reroot_equal_the_restatement(libs, tid, mid):
    """Cases 1 and 2: three moves by the most visited action with reroot between the rounds; leaves after every call,
    results after every round and after every reroot agree bit for bit; what reroot keeps is the old child's edge
    statistics, and the new root's emitted rows are the reference-pinned rows of the position behind the move."""
    S = sims(tid)
    game_, pos = start(libs, tid, mid)
    pair = Pair(libs, game_, pos, S, 1.25, 2 * S + 1)
    kept_any = False
    for move in range(3):
        (visits, values, action, nodes), _ = pair.round()
        a = int(action[0])
        assert a >= 0 and pair.tree.root.pos.mask[a]
        assert visits.sum() >= S  # (the kept visits count)
        child = pair.tree.root.child[a]
        after, _ = game_.at(pair.tree.root.pos.key[0] + (a,))
        obs, mask, status = pair.reroot(a)
        got = pair.host.result()
        if after.done:
            assert status[0] == 2 and got[2][0] == -1 and not got[0].any() and not got[1].any()
            break
        # the invariant that needs no restatement: every simulation through the edge but the one that made the child
        assert got[0].sum() == visits[0][a] - 1, (tid, move)
        assert got[3][0] <= nodes[0] - 1 and got[3][0] >= 1
        kept_any = kept_any or got[3][0] > 1
        # the old child's edge statistics, seen from the new root's mover
        sign = F(1 if after.mover == 0 else -1)
        assert np.array_equal(got[0][0], np.array(child.v, np.int32))
        assert np.array_equal(bits(got[1][0]), bits(np.array([sign * F(w) for w in child.w0], F)))
        # the emitted rows: the reference-pinned rows of the seat to move
        assert status[0] == 0
        assert np.array_equal(obs[0].astype(bool), after.obs) and np.array_equal(mask[0].astype(bool), after.mask)
    assert kept_any or (after.done and move == 0)  # (a mid-game TicTacToe row may end with the first move)
    pair.close()


@pytest.mark.parametrize("tid", GAMES)
def test_reroot_by_an_untried_move_is_a_fresh_tree(libs, tid):
    """Case 3: after a round of 3 simulations most root moves have no child; reroot by one of them (with a longer next
    round), and from then on leaves and results equal a session begun on that position."""
    S2 = sims(tid)
    game_, pos = start(libs, tid, False)
    pair = Pair(libs, game_, pos, 3, 1.25, S2 + 1)
    (visits, _, _, _), _ = pair.round()
    a = int(np.flatnonzero(pos.mask & (visits[0] == 0))[-1])
    assert a not in pair.tree.root.child
    pair.reroot(a, S2)
    after, _ = game_.at(pos.key[0] + (a,))
    fresh = base.HostSession(libs, tid, [after], S2, 1.25)
    assert pair.host.result()[3][0] == 1 and not pair.host.result()[0].any()
    for t in range(S2 + 1):
        for x, y in zip(pair.host.leaves(), fresh.leaves()):
            assert np.array_equal(x, y), (tid, t)
        priors, values = stand_in(*pair.host.leaves()[:2])
        assert pair.host.advance(priors, values) == 0 and fresh.advance(priors, values) == 0
        pair.tree.advance(priors[0], values[0])
        for x, y in zip(pair.host.result(), fresh.result()):
            assert np.array_equal(x, y), (tid, t)
    same_result(pair.host.result(), pair.tree.result(), tid)
    fresh.close()
    pair.close()


def flat(denominator):
    def evaluate(obs, mask):
        return (mask > 0).astype(F) / F(denominator), np.zeros(len(mask), F)
    return evaluate


def test_roots_that_are_over(libs):
    """Case 4: reroot into a finished child (TicTacToe, a win in one) gives status 2, action -1 and zero rows, for the
    rest of the session; a root that was over at begin ignores its action."""
    game_ = base.Replayed(libs, "TicTacToe-v1", column=0)
    pos, _ = game_.at([0, 3, 1, 4])
    assert not pos.done and pos.mask[2]
    pair = Pair(libs, game_, pos, 24, 1.25, 49, evaluate=flat(8.0))
    (visits, values, action, nodes), seen = pair.round()
    assert action[0] == 2 and 1 in seen and pair.tree.root.child[2].pos.done
    obs, mask, status = pair.reroot(2)
    assert status[0] == 2 and not obs.any() and not mask.any()
    for _ in range(2):  # ... and through another round and another reroot
        (visits, values, action, nodes), seen = pair.round()
        assert action[0] == -1 and not visits.any() and not values.any() and set(seen) == {2}
        pair.reroot(0)
    pair.close()

    over = base.Replayed(libs, "TicTacToe-v1", column=0)
    done_pos = over.fixture_row(int(np.flatnonzero(over.g["done"][:, 0])[0]))
    assert done_pos.done
    for a in (0, 8, -1, 9, 1 << 30):  # (ignored: out of range, too)
        host = RerootSession(libs, "TicTacToe-v1", [done_pos, pos], 2, 1.25, 5)
        for t in range(3):
            assert host.advance(*flat(8.0)(*host.leaves()[:2])) == 0
        assert host.reroot([a, 5], 2) == 0
        assert host.status.tolist() == [2, 0] and not host.obs[0].any() and host.mask[1].sum() == 4
        visits, values, action, nodes = host.result()
        assert action[0] == -1 and not visits[0].any() and not values[0].any()
        host.close()
    # an action out of range ends a running root (the engine's host form refuses it; the device form cannot look)
    host = RerootSession(libs, "TicTacToe-v1", [pos], 2, 1.25, 5)
    for t in range(3):
        assert host.advance(*flat(8.0)(*host.leaves()[:2])) == 0
    assert host.reroot([9], 2) == 0 and host.status[0] == 2 and host.result()[2][0] == -1
    host.close()
    # an illegal move (cell 3 is taken) ends the game in Step: the root is over
    host = RerootSession(libs, "TicTacToe-v1", [pos], 2, 1.25, 5)
    for t in range(3):
        assert host.advance(*flat(8.0)(*host.leaves()[:2])) == 0
    assert not pos.mask[3] and host.reroot([3], 2) == 0 and host.status[0] == 2 and host.result()[2][0] == -1
    host.close()


@pytest.mark.parametrize("tid", GAMES)
def test_capacity_ends_a_root_without_an_error(libs, tid):
    """Case 5: nodes = S + 1.  After a reroot that keeps n nodes the next round of S simulations runs out of nodes: the
    root goes idle once count == C, the visits grow by exactly the descents made, no error is reported (Pair.round
    asserts rc == 0 on every call), and the restatement agrees call for call."""
    S = sims(tid)
    game_, pos = start(libs, tid, False)
    pair = Pair(libs, game_, pos, S, 1.25, S + 1)
    (visits, _, action, nodes), _ = pair.round()
    assert nodes[0] == S + 1 or tid == "TicTacToe-v1"
    pair.reroot(int(action[0]))
    kept_visits, n = int(pair.host.result()[0].sum()), int(pair.host.result()[3][0])
    assert n > 1
    (visits, _, _, nodes), seen = pair.round()
    descents = sum(1 for s in seen[1:] if s != 2)  # every leaf handed out after the root's own evaluation
    assert visits.sum() == kept_visits + descents
    assert descents < S, "the capacity did not bind"
    assert nodes[0] == S + 1 and seen[-1] == 2
    if 1 not in seen:  # every descent made a node
        assert descents == S + 1 - n
        assert seen == [0] * (descents + 1) + [2] * (S - descents)
    else:
        assert seen.count(2) > 0 and 2 not in seen[:seen.index(2)]
    pair.close()


@pytest.mark.parametrize("tid,nodes", [("ConnectFour-v1", 513), ("ConnectFour-v1", 2049), ("ConnectFour-v1", 8192),
                                       ("Hex-v1", 513), ("Hex-v1", 2049)])
def test_capacities_above_512_and_2048_nodes(libs, tid, nodes):
    """The capacities at which the kernel's mark / rank table is the 2048- and the 8192-entry one (513, 2049; 8192 is
    the limit): a round of 8 simulations, a reroot by the chosen move, a second round -- harness against restatement
    after every call, as everywhere in Pair."""
    S = 8
    game_, pos = start(libs, tid, True)
    pair = Pair(libs, game_, pos, S, 1.25, nodes)
    (visits, _, action, _), _ = pair.round()
    a = int(action[0])
    assert visits[0][a] >= 1  # the most visited of S >= 1 visits: it has a child, so the table path runs
    pair.reroot(a)
    kept = pair.host.result()
    if pair.host.status[0] == 0:  # (else the move ended the game)
        assert kept[0].sum() == visits[0][a] - 1 and 1 <= kept[3][0] <= visits[0][a]
        (after, _, _, used), _ = pair.round()
        assert after.sum() == kept[0].sum() + S and used[0] <= kept[3][0] + S
    pair.close()


@pytest.mark.parametrize("played", ["swap", "cell"])
def test_hex_second_slots_and_the_swap(libs, played):
    """Case 6: Hex one stone in, flat priors, S > 121, so every root move has a child: play the swap (action 121) or a
    cell >= 64 -- the second action slot of a lane in reroot's root lookup, copy and remap."""
    game_ = base.Replayed(libs, "Hex-v1", column=0)
    pos, _ = game_.at([60])
    assert pos.mask[121] and pos.mask.sum() == 121
    pair = Pair(libs, game_, pos, 124, 1.25, 249, evaluate=flat(128.0))
    (visits, _, _, nodes), _ = pair.round()
    assert (visits[0][pos.mask] >= 1).all() and len(pair.tree.root.child) == 121
    a = 121 if played == "swap" else 64 + int(np.argmax(visits[0][64:121]))
    obs, mask, status = pair.reroot(a, 12)
    got = pair.host.result()
    assert status[0] == 0 and got[0].sum() == visits[0][a] - 1 and got[3][0] == visits[0][a]
    (visits, _, action, _), _ = pair.round()
    assert visits.sum() == got[0].sum() + 12
    pair.reroot(int(action[0]))
    pair.round()
    pair.close()


def test_othello_forced_pass_as_the_played_move(libs):
    """Case 6: the pass (action 64) is lane 0's second slot; it is the root's only move, so its subtree is the whole
    tree but the root."""
    game_ = base.Replayed(libs, "Othello-v1", column=0)
    rng = np.random.default_rng(5)
    found = None
    for _ in range(400):
        seq = []
        pos, _ = game_.at(seq)
        while not pos.done and found is None:
            if pos.mask[64]:
                found = pos
                break
            seq.append(int(rng.choice(np.flatnonzero(pos.mask))))
            pos, _ = game_.at(seq)
        if found is not None:
            break
    assert found is not None and found.mask.sum() == 1, "no forced pass found"
    pair = Pair(libs, game_, found, 24, 1.25, 49)
    (visits, _, action, nodes), _ = pair.round()
    assert action[0] == 64 and visits[0][64] == 24
    pair.reroot(64)
    got = pair.host.result()
    assert got[0].sum() == 23 and got[3][0] == nodes[0] - 1
    pair.round()
    pair.close()


@pytest.mark.parametrize("tid", GAMES)
def test_a_session_that_is_never_rerooted_is_todays(libs, tid):
    """Case 8: nodes = S + 1 and no reroot: leaves and results equal pgx_guided_host.cpp's, call for call."""
    S = sims(tid)
    game_, pos = start(libs, tid, True)
    over = game_.fixture_row(int(np.flatnonzero(game_.g["done"][:, 2])[0]))
    poss = [pos, over, game_.fixture_row(0)]
    for nodes in (S + 1, 2 * S + 1):
        new = RerootSession(libs, tid, poss, S, 1.25, nodes)
        ref = base.HostSession(libs, tid, poss, S, 1.25)
        for t in range(S + 1):
            for x, y in zip(new.leaves(), ref.leaves()):
                assert np.array_equal(x, y), (tid, t)
            priors, values = stand_in(*new.leaves()[:2])
            assert new.advance(priors, values) == 0 and ref.advance(priors, values) == 0
            for x, y in zip(new.result(), ref.result()):
                assert np.array_equal(x, y), (tid, t)
        new.close()
        ref.close()


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_harness_refusals(libs):
    pos = base.Replayed(libs, "ConnectFour-v1", column=1).fixture_row(0)
    for S, nodes in ((4, 4), (4, 8193), (0, 4), (4097, 4200)):
        RerootSession(libs, "ConnectFour-v1", [pos], S, 1.25, nodes, want_rc=-6)
    host = RerootSession(libs, "ConnectFour-v1", [pos], 4, 1.25, 8)
    for t in range(5):
        assert host.reroot([3], 4) == -5  # before the round's last advance
        assert host.advance(*stand_in(*host.leaves()[:2])) == 0
    for s2 in (0, -1, 8, 4097):  # outside 1 .. 4096, or S2 + 1 > C
        assert host.reroot([3], s2) == -6
    assert host.reroot([3], 7) == 0 and host.status[0] == 0
    assert host.reroot([3], 7) == -5  # a new round has begun
    host.close()


def test_check_guided_nodes_and_reroot():
    from envpool_amd.core import native

    assert native.check_guided_nodes(64, None) == 65 and native.check_guided_nodes(64, 0) == 65
    assert native.check_guided_nodes(64, 65) == 65 and native.check_guided_nodes(4096, 8192) == 8192
    for S, nodes in ((64, 64), (64, 8193), (64, -1), (4096, 4096)):
        with pytest.raises(ValueError, match="guided_begin: nodes"):
            native.check_guided_nodes(S, nodes)
    acts = native.check_guided_reroot([[2], [0]], 2, 9, 24, 49)
    assert acts.dtype == np.int32 and acts.tolist() == [2, 0] and acts.flags.c_contiguous
    native.check_guided_reroot([8, 8], 2, 9, 48, 49)
    for actions, k, s2, nodes in (([2], 2, 24, 49), ([2, 0, 1], 2, 24, 49), ([2, 9], 2, 24, 49), ([-1, 0], 2, 24, 49),
                                  ([2, 0], 2, 0, 49), ([2, 0], 2, 4097, 8192), ([2, 0], 2, 49, 49)):
        with pytest.raises(ValueError, match="guided_reroot"):
            native.check_guided_reroot(actions, k, 9, s2, nodes)
    # the device form cannot look at its rows: only the round's length is checked
    assert native.check_guided_reroot(None, 2, 9, 24, 49, device=True) is None
    with pytest.raises(ValueError, match="guided_reroot"):
        native.check_guided_reroot(None, 2, 9, 49, 49, device=True)


class _Recorder(base._Recorder):
    """A pool that records the guided calls it gets, reroot and the capacity among them."""

    def guided_begin(self, env_ids, simulations, c_puct, nodes=None):
        out = super().guided_begin(env_ids, simulations, c_puct)
        self.calls[-1] += (nodes,)
        return out

    def guided_reroot(self, actions, simulations):
        self.calls.append(("reroot", np.asarray(actions).tolist(), simulations))
        return self._leaves()


def test_wrapper_checks_come_before_the_native_call():
    from envpool_amd.pgx import OthelloGymnasiumEnvPool

    env = object.__new__(OthelloGymnasiumEnvPool)
    env._pool = _Recorder()
    ids = np.array([2, 0, 1], np.int32)
    for nodes in (3, 8193, -5):
        with pytest.raises(ValueError, match="guided_begin: nodes"):
            env.guided_search(ids, simulations=3, nodes=nodes)
    with pytest.raises(ValueError, match="gumbel"):
        env.guided_search(ids, simulations=3, policy="gumbel", nodes=9)
    assert env._pool.calls == []
    gs = env.guided_search(ids, simulations=3, c_puct=0.5, nodes=9)
    assert env._pool.calls == [("begin", [2, 0, 1], 3, 0.5, 9)]

    def evaluate(obs, mask, status):
        return np.zeros((3, 65), np.float32), np.zeros(3, np.float32)

    with pytest.raises(ValueError, match="round is not complete"):
        gs.reroot([1, 2, 3])
    gs.advance(*evaluate(*gs.leaves))
    with pytest.raises(ValueError, match="round is not complete"):
        gs.reroot([1, 2, 3])
    out = gs.run(evaluate, close=False)
    assert out._fields == ("visits", "values", "action") and gs.calls == 4
    assert [c[0] for c in env._pool.calls] == ["begin"] + ["advance"] * 4 + ["result"]  # (still open)
    leaves = gs.reroot([1, 2, 3])
    assert env._pool.calls[-1] == ("reroot", [1, 2, 3], 3) and gs.calls == 0 and leaves is gs.leaves
    gs.run(evaluate, close=False)
    gs.reroot([4, 5, 6], simulations=5)
    assert env._pool.calls[-1] == ("reroot", [4, 5, 6], 5) and gs.simulations == 5 and gs.calls == 0
    gs.run(evaluate)
    assert [c[0] for c in env._pool.calls][-8:] == ["advance"] * 6 + ["result", "end"]
    with pytest.raises(ValueError, match="closed"):
        gs.reroot([1, 2, 3])
