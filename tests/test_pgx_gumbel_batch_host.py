"""PGX Gumbel search, a halving level per launch, CPU side: the batch sessions of envpool_amd/csrc/pgx_gumbel.hip.h
built for the host by g++ (tests/cpu_harness/pgx_gumbel_batch_host.cpp, which walks a wave's lanes as loops) against
the contract restated in numpy float32 (pgx_gumbel_batch_util.py) on positions of the reference-pinned replays; every
consequence the contract states (B = 1 is the plain session, disjoint slots, one node per descent, the number of
advances of a round, the visit counts, constant values give the plain session's results); and the argument checks of
the Python layers, which come before any native call."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from pgx_gumbel_batch_util import GumbelBatchTree, advances_of_a_round, level_left, levels
from pgx_gumbel_util import gumbel_noise, sequence_of_considered_visits, stand_in_logits, visit_multiset, wild_logits
from pgx_util import ACTIONS, CODE, game
from test_pgx_guided_host import Replayed, mid_row
from test_pgx_gumbel_host import HostSession

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMES = ["TicTacToe-v1", "ConnectFour-v1", "Hex-v1", "Othello-v1"]
F = np.float32
FLAGS = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"]  # no fast-math, no contraction


def _build(tmp, source, name):
    out = str(tmp / name)
    subprocess.run(FLAGS + ["-shared", "-fPIC", os.path.join(ROOT, "tests", "cpu_harness", source), "-o", out],
                   check=True)
    return ctypes.CDLL(out)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    """(the PGX host harness, the plain Gumbel harness, the batch harness)"""
    tmp = tmp_path_factory.mktemp("pgx_gumbel_batch")
    plain = _build(tmp, "pgx_gumbel_host.cpp", "libpgxgumbelhost.so")
    plain.pgx_gumbel_begin.restype = ctypes.c_void_p
    plain.pgx_gumbel_result.restype = None
    plain.pgx_gumbel_end.restype = None
    batch = _build(tmp, "pgx_gumbel_batch_host.cpp", "libpgxgumbelbatchhost.so")
    batch.pgx_gumbel_batch_begin.restype = ctypes.c_void_p
    batch.pgx_gumbel_batch_result.restype = None
    batch.pgx_gumbel_batch_end.restype = None
    return _build(tmp, "pgx_host.cpp", "libpgxhost.so"), plain, batch


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


class BatchSession:
    """The harness's batch session over the roots `poss` (Pos with key = (seq, hidden words)): the leaf arrays carry
    the slot axis, [n, B, ...]."""

    def __init__(self, libs, tid, poss, simulations, considered, batch, gumbel, c_visit=50.0, c_scale=0.1):
        self.lib, self.n, self.n_act, self.B = libs[2], len(poss), ACTIONS[game(tid)], batch
        hid = np.ascontiguousarray(np.stack([p.key[1] for p in poss]), np.int32)
        done = np.array([p.done for p in poss], np.uint8)
        gumbel = np.ascontiguousarray(gumbel, F)
        assert gumbel.shape == (self.n, self.n_act)
        self.obs = np.full((self.n, batch) + poss[0].obs.shape, 7, np.uint8)
        self.mask = np.full((self.n, batch, self.n_act), 7, np.uint8)
        self.status = np.full((self.n, batch), 7, np.uint8)
        rc = ctypes.c_int(-9)
        self.h = self.lib.pgx_gumbel_batch_begin(CODE[game(tid)], self.n, _ptr(hid), _ptr(done), simulations,
                                                 considered, batch, ctypes.c_float(c_visit), ctypes.c_float(c_scale),
                                                 _ptr(gumbel), _ptr(self.obs), _ptr(self.mask), _ptr(self.status),
                                                 ctypes.byref(rc))
        assert rc.value == 0 and self.h

    def leaves(self):
        return self.obs.copy(), self.mask.copy(), self.status.copy()

    def advance(self, logits, values):
        logits, values = np.ascontiguousarray(logits, F), np.ascontiguousarray(values, F)
        assert logits.shape == (self.n, self.B, self.n_act) and values.shape == (self.n, self.B)
        return self.lib.pgx_gumbel_batch_advance(ctypes.c_void_p(self.h), _ptr(logits), _ptr(values), _ptr(self.obs),
                                                 _ptr(self.mask), _ptr(self.status))

    def result(self):
        visits, values = np.full((self.n, self.n_act), -7, np.int32), np.full((self.n, self.n_act), -7, F)
        action, nodes = np.full(self.n, -7, np.int32), np.zeros(self.n, np.int32)
        weights = np.full((self.n, self.n_act), -7, F)
        self.lib.pgx_gumbel_batch_result(ctypes.c_void_p(self.h), _ptr(visits), _ptr(values), _ptr(action),
                                         _ptr(weights), _ptr(nodes))
        return visits, values, action, weights, nodes

    def close(self):
        self.lib.pgx_gumbel_batch_end(ctypes.c_void_p(self.h))
        self.h = None


def flat(evaluate):
    """An evaluator of [n, ...] rows as one of [n, B, ...] rows."""
    def go(obs, mask):
        n, b = mask.shape[:2]
        logits, values = evaluate(obs.reshape((n * b,) + obs.shape[2:]), mask.reshape(n * b, -1))
        return logits.reshape(n, b, -1), values.reshape(n, b)
    return go


def same_result(got, ref, where):
    assert np.array_equal(got[0], ref[0]), (where, got[0], ref[0])
    assert np.array_equal(bits(got[1]), bits(ref[1])), (where, got[1], ref[1])
    assert got[2] == ref[2], (where, got[2], ref[2])
    assert np.array_equal(bits(got[3]), bits(ref[3])), (where, got[3], ref[3])
    assert got[4] == ref[4], where


def both(libs, game_, pos, simulations, considered, batch, gumbel, evaluate=stand_in_logits, **consts):
    """The numpy restatement and the harness from `pos`, fed the same evaluator, compared after every call -- the
    leaves of every slot and the result, bit for bit -- with what every round must show whatever its arithmetic.
    Returns (the harness's final result, the statuses seen per call)."""
    tree = GumbelBatchTree(pos, pos.done, game_.expand, simulations, considered, batch, gumbel, **consts)
    host = BatchSession(libs, game_.tid, [pos], simulations, considered, batch, gumbel[None, :], **consts)
    where = (game_.tid, simulations, considered, batch)
    m_eff = min(considered, int(pos.mask.sum()))
    seen, total = [], 0
    evaluate = flat(evaluate)
    for t in range(simulations + 1):
        obs, mask, status = host.leaves()
        want = tree.leaves()
        for j in range(batch):
            assert status[0, j] == want[j][2], (where, t, j)
            assert np.array_equal(obs[0, j].astype(bool), want[j][0]), (where, t, j)
            assert np.array_equal(mask[0, j].astype(bool), want[j][1]), (where, t, j)
            if status[0, j] != 0:
                assert not obs[0, j].any() and not mask[0, j].any()
        live = [j for j in range(batch) if status[0, j] != 2]
        assert live == list(range(len(live)))  # the pending slots come first
        # disjoint slots: different root actions, no node but the root in two paths
        paths = [tree.slots[j]["path"] for j in live]
        if t > 0:
            assert len({p[0][1] for p in paths}) == len(paths) and all(p[0][0] == 0 for p in paths), (where, t)
            inner = [n for p in paths for n, _ in p[1:]] + [tree.slots[j]["pending"] for j in live]
            assert len(set(inner)) == len(inner), (where, t)
        if not pos.done and total < simulations:
            assert len(live) >= 1, (where, t)  # while t < S every advance completes a simulation
            if t > 0:
                assert len(live) == min(batch, level_left(m_eff, simulations, total)), (where, t)
        seen.append(status[0].tolist())
        logits, values = evaluate(obs, mask)
        assert host.advance(logits, values) == 0
        tree.advance(logits[0], values[0])
        got, ref = host.result(), tree.result()
        same_result([x[0] for x in got], ref, (where, t))
        total = int(got[0].sum())
        assert total == seen_total(seen, pos), (where, t)  # every leaf handed out below the root is a simulation
        assert got[4][0] <= simulations + 1  # at most one node per descent
    assert (host.status == 2).all() and not host.obs.any() and not host.mask.any()
    assert host.advance(logits, values) == -4  # a call number above S
    out = host.result()
    host.close()
    if not pos.done:
        assert out[0].sum() == simulations and (out[0][0][~pos.mask] == 0).all()
        assert sorted(out[0][0][out[0][0] > 0].tolist()) == [c for c in visit_multiset(m_eff, simulations) if c > 0]
        pending = [t for t, st in enumerate(seen) if any(x != 2 for x in st)]
        assert pending == list(range(advances_of_a_round(m_eff, simulations, batch))), (where, pending)
    return out, seen


def seen_total(seen, pos):
    """The simulations that the answers to the leaves of the calls in `seen` complete: every leaf but the root's."""
    return 0 if pos.done else sum(sum(x != 2 for x in st) for st in seen[1:])


def seeded(tid, seed=7):
    return gumbel_noise(seed, 1, ACTIONS[game(tid)])[0]


def mid_pos(libs, tid, column=2):
    game_ = Replayed(libs, tid, column=column)
    pos = game_.fixture_row(mid_row(game_.g, column))
    assert not pos.done
    return game_, pos


# ---- the header's walk of the level ---------------------------------------------------------------------------------
def test_level_left_walk_equals_the_sequence(libs):
    left, walk = libs[2].pgx_gumbel_batch_level_left, libs[2].pgx_gumbel_batch_considered_visit
    for m in range(1, max(ACTIONS.values()) + 1):
        for s in (1, 2, 7, 16, 20, 33, 64):
            seq = sequence_of_considered_visits(m, s)
            assert [walk(m, s, t) for t in range(s)] == seq
            assert [left(m, s, t) for t in range(s)] == [level_left(m, s, t) for t in range(s)], (m, s)
            assert sum(levels(m, s)) == s
    assert levels(16, 32) == [16, 8, 4, 4] and levels(16, 20) == [16, 4] and levels(1, 3) == [1, 1, 1]
    # the issue's arithmetic: model calls of a round
    assert advances_of_a_round(16, 32, 16) == 5 and advances_of_a_round(16, 64, 16) == 16
    assert advances_of_a_round(16, 32, 1) == 33 and advances_of_a_round(16, 32, 4) == 1 + 4 + 2 + 1 + 1


# ---- the three implementations agree --------------------------------------------------------------------------------
@pytest.mark.parametrize("considered", [4, 8, 16])
@pytest.mark.parametrize("simulations", [16, 32])
@pytest.mark.parametrize("batch", [2, 4, 16])
@pytest.mark.parametrize("tid", GAMES)
def test_host_session_equals_the_numpy_restatement(libs, tid, batch, simulations, considered):
    game_, pos = mid_pos(libs, tid)
    out, seen = both(libs, game_, pos, simulations, considered, batch, seeded(tid))
    assert out[4][0] <= simulations + 1
    if tid == "Hex-v1":
        assert pos.mask[64:].any()  # the second slot of a lane is live


def test_a_level_larger_than_the_batch_and_a_cut_last_level(libs):
    """m = 16 at B = 4: the first level takes four launches; S = 20 and 37 are no sums of whole levels."""
    for tid in ("Hex-v1", "Othello-v1"):
        game_ = Replayed(libs, tid, column=1)
        pos = game_.fixture_row(0)
        m_eff = min(16, int(pos.mask.sum()))
        for simulations in (20, 37):
            _, seen = both(libs, game_, pos, simulations, 16, 4, seeded(tid, 3))
            sizes = [sum(x != 2 for x in st) for st in seen[1:]]
            want = [min(4, size - q) for size in levels(m_eff, simulations) for q in range(0, size, 4)]
            assert [s for s in sizes if s] == want, (tid, simulations)
    assert levels(16, 20)[-1] < 8 and levels(16, 37)[-1] == 1


# ---- the consequences -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tid", GAMES)
def test_batch_one_is_the_plain_session(libs, tid):
    """B = 1 against the plain harness, call for call, bit for bit, in leaves and in results."""
    game_, pos = mid_pos(libs, tid)
    start = Replayed(libs, tid, column=1).fixture_row(0)
    n_act = ACTIONS[game(tid)]
    for simulations, considered, evaluate in ((16, 4, stand_in_logits), (33, 16, stand_in_logits),
                                              (16, n_act, wild_logits)):
        poss = [pos, start]
        noise = gumbel_noise(5, 2, n_act)
        plain = HostSession(libs, tid, poss, simulations, considered, noise)
        batch = BatchSession(libs, tid, poss, simulations, considered, 1, noise)
        for t in range(simulations + 1):
            a, b = plain.leaves(), batch.leaves()
            for x, y in zip(a, b):
                assert np.array_equal(x, y[:, 0]), (tid, t)
            logits, values = evaluate(a[0], a[1])
            assert plain.advance(logits, values) == 0
            assert batch.advance(logits[:, None], values[:, None]) == 0
            for x, y in zip(plain.result(), batch.result()):
                assert np.array_equal(x.view(np.uint32) if x.dtype == F else x, y.view(np.uint32) if y.dtype == F else y)
        assert plain.advance(logits, values) == -4 and batch.advance(logits[:, None], values[:, None]) == -4
        plain.close()
        batch.close()


def zero_values(obs, mask):
    logits, values = stand_in_logits(obs, mask)
    return logits, np.zeros_like(values)


@pytest.mark.parametrize("tid", ["Hex-v1", "Othello-v1", "ConnectFour-v1"])
def test_constant_values_give_the_plain_sessions_results(libs, tid):
    """Values all 0, no finished game reached: sigma is 0 everywhere, the root order is fixed, and every B gives the
    plain session's visits, values, action, weights and node count, bit for bit."""
    start = Replayed(libs, tid, column=1).fixture_row(0)
    n_act = ACTIONS[game(tid)]
    noise = gumbel_noise(9, 1, n_act)
    simulations, considered = 32, 16
    plain = HostSession(libs, tid, [start], simulations, considered, noise)
    for _ in range(simulations + 1):
        obs, mask, status = plain.leaves()
        assert status[0] != 1
        assert plain.advance(*zero_values(obs, mask)) == 0
    want = plain.result()
    plain.close()
    for batch in (2, 4, 16, 32):
        host = BatchSession(libs, tid, [start], simulations, considered, batch, noise)
        calls = 0
        while (host.status != 2).any():
            obs, mask, status = host.leaves()
            assert not (status == 1).any()  # the condition is checked, not assumed
            assert host.advance(*flat(zero_values)(obs, mask)) == 0
            calls += 1
        assert calls == advances_of_a_round(min(considered, int(start.mask.sum())), simulations, batch)
        for x, y in zip(want, host.result()):
            assert np.array_equal(x.view(np.uint32) if x.dtype == F else x, y.view(np.uint32) if y.dtype == F else y)
        host.close()


def test_other_values_differ_from_the_plain_session(libs):
    """With values that vary sigma moves inside a level, which only the plain session sees: the two searches part.
    (What the batch session then gives is pinned by the restatement and the harness, above.)"""
    differ = 0
    for tid in GAMES[1:]:
        game_, pos = mid_pos(libs, tid)
        noise = seeded(tid)
        plain = HostSession(libs, tid, [pos], 32, 16, noise[None, :])
        for _ in range(33):
            obs, mask, _ = plain.leaves()
            assert plain.advance(*stand_in_logits(obs, mask)) == 0
        want = plain.result()
        plain.close()
        out, _ = both(libs, game_, pos, 32, 16, 16, noise)
        assert sorted(out[0][0].tolist()) == sorted(want[0][0].tolist())  # the same visit counts ...
        differ += not np.array_equal(bits(out[1]), bits(want[1]))          # ... through other leaves
    assert differ > 0


def test_later_advances_change_nothing(libs):
    game_, pos = mid_pos(libs, "ConnectFour-v1")
    host = BatchSession(libs, game_.tid, [pos], 16, 8, 4, seeded(game_.tid)[None, :])
    calls = 0
    while (host.status != 2).any():
        obs, mask, _ = host.leaves()
        assert host.advance(*flat(stand_in_logits)(obs, mask)) == 0
        calls += 1
    done = host.result()
    junk = np.full((1, 4, 7), 3.0, F), np.full((1, 4), 0.5, F)
    for _ in range(calls, 17):
        assert host.advance(*junk) == 0
        assert (host.status == 2).all() and not host.obs.any() and not host.mask.any()
        for x, y in zip(done, host.result()):
            assert np.array_equal(x, y)
    assert host.advance(*junk) == -4
    host.close()


# ---- further cases --------------------------------------------------------------------------------------------------
def forced_pass(libs):
    game_ = Replayed(libs, "Othello-v1", column=0)
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


def test_fewer_legal_actions_than_considered(libs):
    """Othello's forced pass: m_eff = 1, every simulation a level of its own, one slot per launch whatever B.  And a
    late TicTacToe position with three empty cells, where most simulations end in a finished game."""
    game_, pos = forced_pass(libs)
    for batch in (2, 16):
        out, seen = both(libs, game_, pos, 7, 16, batch, seeded("Othello-v1"))
        assert out[0][0][64] == 7 and out[2][0] == 64 and out[3][0][64] == 1
        assert all(sum(x != 2 for x in st) == 1 for st in seen)  # S + 1 advances of one leaf
    game_ = Replayed(libs, "TicTacToe-v1", column=0)
    pos, _ = game_.at([0, 1, 2, 4, 3, 5])
    assert not pos.done and pos.mask.sum() == 3
    for batch, considered in ((2, 2), (4, 9), (16, 3)):
        out, seen = both(libs, game_, pos, 16, considered, batch, seeded("TicTacToe-v1"))
        assert any(1 in st for st in seen)


def test_a_finished_child_is_visited_again_in_later_levels(libs):
    """A root action that ends the game: its child is a finished node, reached again in every later level it
    survives -- status 1 each time, term0 backed up each time, no node made."""
    game_ = Replayed(libs, "TicTacToe-v1", column=0)
    pos, _ = game_.at([0, 3, 1, 4])  # the mover wins with cell 2
    assert not pos.done and pos.mask[2]
    noise = np.zeros(9, F)
    noise[2] = 5.0  # the winning move stays among the considered actions
    out, seen = both(libs, game_, pos, 16, 4, 4, noise)
    ones = sum(st.count(1) for st in seen)
    assert out[0][0][2] >= 2 and ones >= out[0][0][2]
    assert out[1][0][2] == out[0][0][2]  # every visit of the winning move is worth +1 for the mover


def test_a_root_that_is_over_at_begin(libs):
    game_ = Replayed(libs, "TicTacToe-v1", column=0)
    over = game_.fixture_row(int(np.flatnonzero(game_.g["done"][:, 0])[0]))
    assert over.done
    out, seen = both(libs, game_, over, 7, 4, 4, seeded("TicTacToe-v1"))
    assert out[2][0] == -1 and not out[0].any() and not out[3].any() and {x for st in seen for x in st} == {2}


def test_hex_every_action_considered_at_the_widest_batch(libs):
    """m = A = 122, B = 32, S = 64: one level of 64 simulations in two launches, picks from both slots of a lane."""
    game_ = Replayed(libs, "Hex-v1", column=1)
    pos = game_.fixture_row(0)
    out, seen = both(libs, game_, pos, 64, 122, 32, seeded("Hex-v1", 11))
    assert [sum(x != 2 for x in st) for st in seen[:4]] == [1, 32, 32, 0]
    assert out[0][0].max() == 1 and out[0][0][64:].any() and out[0][0][:64].any()


def test_rows_are_cleaned_per_slot_and_zero_noise(libs):
    """Logits and values that are not finite or out of range count as 0 in the slot they arrive in, and only there;
    all-zero noise is the evaluation mode."""
    game_, pos = mid_pos(libs, "ConnectFour-v1")

    def dirty(obs, mask):
        logits, values = stand_in_logits(obs, mask)
        logits[1::2, 0], logits[1::2, 3] = np.nan, 2e30
        values[1::2] = 1.5
        return logits, values

    def zeroed(obs, mask):
        logits, values = stand_in_logits(obs, mask)
        logits[1::2, 0], logits[1::2, 3] = 0.0, 0.0
        values[1::2] = 0.0
        return logits, values

    noise = np.zeros(7, F)
    a, _ = both(libs, game_, pos, 16, 4, 4, noise, evaluate=dirty)
    b, _ = both(libs, Replayed(libs, "ConnectFour-v1", column=2), pos, 16, 4, 4, noise, evaluate=zeroed)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    c, _ = both(libs, Replayed(libs, "ConnectFour-v1", column=2), pos, 16, 4, 4, noise)
    assert not np.array_equal(bits(a[1]), bits(c[1]))  # the dirty slots did matter
    both(libs, game_, pos, 16, 7, 4, noise, evaluate=wild_logits, c_visit=3e38, c_scale=3e38)


def test_several_roots_in_one_session(libs):
    """Rows are independent: a session over three roots, one of them over, equals three sessions of one."""
    game_ = Replayed(libs, "ConnectFour-v1", column=2)
    g = game_.g
    over = int(np.flatnonzero(g["done"][:, 2])[0])
    poss = [game_.fixture_row(0), game_.fixture_row(over), game_.fixture_row(mid_row(g, 2))]
    assert [p.done for p in poss] == [False, True, False]
    noise = gumbel_noise(1, 3, 7)
    many = BatchSession(libs, game_.tid, poss, 16, 4, 4, noise)
    ones = [BatchSession(libs, game_.tid, [p], 16, 4, 4, noise[i:i + 1]) for i, p in enumerate(poss)]
    for _ in range(17):
        obs, mask, status = many.leaves()
        for i, one in enumerate(ones):
            for a, b in zip((obs, mask, status), one.leaves()):
                assert np.array_equal(a[i:i + 1], b)
        logits, values = flat(stand_in_logits)(obs, mask)
        assert many.advance(logits, values) == 0
        for i, one in enumerate(ones):
            assert one.advance(logits[i:i + 1], values[i:i + 1]) == 0
    for i, one in enumerate(ones):
        for a, b in zip(many.result(), one.result()):
            assert np.array_equal(a[i:i + 1], b)
        one.close()
    many.close()


def test_record_layout_and_the_harness_refusals(libs):
    """A 16-byte header and the noise row (A rounded up to whole 16-byte words), then B slots of 16 bytes and the
    path; a batch outside 1 .. 32 is refused."""
    lib = libs[2]
    for name, n_act in ACTIONS.items():
        one = lib.pgx_gumbel_batch_root_bytes(CODE[name], 1)
        slot = lib.pgx_gumbel_batch_root_bytes(CODE[name], 2) - one
        assert one - slot == 16 + 4 * ((n_act + 3) // 4 * 4) and slot % 16 == 0 and slot > 16
        assert lib.pgx_gumbel_batch_root_bytes(CODE[name], 32) == one + 31 * slot
    rc = ctypes.c_int(0)
    for batch in (0, -1, 33):
        assert not lib.pgx_gumbel_batch_begin(0, 1, None, None, 4, 4, batch, ctypes.c_float(50), ctypes.c_float(0.1),
                                              None, None, None, None, ctypes.byref(rc))
        assert rc.value == -5


def test_stand_alone_program_builds_and_runs(libs, tmp_path):
    """-DPGX_GUMBEL_BATCH_MAIN: a few rounds of Hex and Othello as a program of its own (the form that runs under the
    host sanitizers; here it is built plain)."""
    out = str(tmp_path / "gumbel_batch_main")
    src = os.path.join(ROOT, "tests", "cpu_harness", "pgx_gumbel_batch_host.cpp")
    subprocess.run(FLAGS + ["-DPGX_GUMBEL_BATCH_MAIN", src, "-o", out], check=True)
    run = subprocess.run([out], check=True, capture_output=True, text=True)
    lines = run.stdout.splitlines()
    assert len(lines) == 6 and all("advances" in x for x in lines)
    assert all(" 3 advances" in x and "nodes 65 65" in x for x in lines[:3])  # Hex: 1 + ceil(64 / 32)


# ---- argument checks ------------------------------------------------------------------------------------------------
def test_check_gumbel_batch():
    from envpool_amd.core import native

    assert native.check_gumbel_batch(None) == 0 and native.check_gumbel_batch(1) == 1
    assert native.check_gumbel_batch(np.int64(32)) == 32 and native.GUMBEL_MAX_BATCH == 32
    for bad in (0, -1, 33, 2.5, True):
        with pytest.raises(ValueError, match="gumbel_begin: batch"):
            native.check_gumbel_batch(bad)
    for logits, values in ((np.zeros((2, 4, 3)), np.zeros((2, 4))), (np.zeros((8, 3)), np.zeros(8)),
                           (np.zeros((2, 4, 3)), np.zeros(8))):
        p, v = native.check_gumbel_batch_rows(logits, values, 2, 4, 3)
        assert p.shape == (8, 3) and v.shape == (8,) and p.dtype == F and v.dtype == F and p.flags.c_contiguous
    for logits, values in ((np.zeros((2, 3)), np.zeros(2)), (np.zeros((2, 4, 3)), np.zeros(2)),
                           (np.zeros((4, 2, 3)), np.zeros((4, 2))), (np.zeros((8, 4)), np.zeros(8)),
                           (np.full((8, 3), np.nan), np.zeros(8)), (np.zeros((8, 3)), np.full(8, 2.0))):
        with pytest.raises(ValueError, match="gumbel_advance"):
            native.check_gumbel_batch_rows(logits, values, 2, 4, 3)


class _Recorder:
    """A pool that records the search calls it gets; a batch session's round is over after `rounds` advances."""

    def __init__(self, rounds=3):
        self.calls, self.rounds, self.batch = [], rounds, 0

    def gumbel_actions(self):
        return 65

    def _leaves(self, status):
        lead = (self.k, self.batch) if self.batch else (self.k,)
        return np.zeros(lead + (8, 8, 2), bool), np.zeros(lead + (65,), bool), np.full(lead, status, np.uint8)

    def gumbel_begin(self, gumbel, env_ids, simulations, max_considered, c_visit, c_scale, batch=None):
        self.calls.append(("begin", np.asarray(env_ids).tolist(), simulations, max_considered, batch))
        self.k, self.batch, self.made = len(env_ids), batch or 0, 0
        return self._leaves(0)

    def gumbel_advance(self, logits, values):
        self.calls.append(("advance", np.asarray(logits).shape, np.asarray(values).shape))
        self.made += 1
        return self._leaves(2 if self.made >= self.rounds else 0)

    def gumbel_result(self):
        self.calls.append(("result",))
        return (np.zeros((self.k, 65), np.int32), np.zeros((self.k, 65), F), np.zeros(self.k, np.int32),
                np.zeros((self.k, 65), F))

    def guided_end(self):
        self.calls.append(("end",))


def test_wrapper_checks_come_before_the_native_call():
    from envpool_amd.pgx import OthelloGymnasiumEnvPool

    env = object.__new__(OthelloGymnasiumEnvPool)
    env._pool = _Recorder()
    ids = np.array([2, 0, 1], np.int32)
    for bad in (0, 33, -2, 1.5):
        with pytest.raises(ValueError, match="gumbel_begin: batch"):
            env.gumbel_search(ids, batch=bad)
        with pytest.raises(ValueError, match="gumbel_begin: batch"):
            env.guided_search(ids, policy="gumbel", batch=bad)
    with pytest.raises(ValueError, match="policy='gumbel'"):
        env.guided_search(ids, batch=4)  # PUCT has width, not batch
    with pytest.raises(ValueError, match="width is an argument of policy='puct'"):
        env.gumbel_search(ids, width=4, batch=4)
    with pytest.raises(ValueError, match="width is an argument of policy='puct'"):
        env.guided_search(ids, policy="gumbel", width=4)
    with pytest.raises(ValueError, match="nodes is an argument of policy='puct'"):
        env.guided_search(ids, policy="gumbel", nodes=64, batch=4)
    assert env._pool.calls == []
    gs = env.gumbel_search(ids, simulations=8, batch=1, seed=1)  # batch 1 opens the plain session
    assert env._pool.calls == [("begin", [2, 0, 1], 8, 16, None)] and gs.batch == 1
    assert [x.shape for x in gs.leaves] == [(3, 8, 8, 2), (3, 65), (3,)]
    env._pool.calls.clear()
    gs = env.guided_search(ids, simulations=8, policy="gumbel", max_considered=4, batch=4, seed=1)
    assert env._pool.calls == [("begin", [2, 0, 1], 8, 4, 4)] and gs.batch == 4 and not gs.done
    assert [x.shape for x in gs.leaves] == [(3, 4, 8, 8, 2), (3, 4, 65), (3, 4)]
    seen = []

    def evaluate(obs, mask, status):
        seen.append((obs.shape, mask.shape, status.shape))
        return np.zeros((12, 65), F), np.zeros(12, F)

    out = gs.run(evaluate)  # flattened rows, until done
    assert out._fields == ("visits", "values", "action", "weights")
    assert seen == [((12, 8, 8, 2), (12, 65), (12,))] * 3
    assert [c[0] for c in env._pool.calls] == ["begin"] + ["advance"] * 3 + ["result", "end"]
    assert env._pool.calls[1] == ("advance", (12, 65), (12,))
    with pytest.raises(ValueError, match="closed"):
        gs.advance(np.zeros((3, 4, 65), F), np.zeros((3, 4), F))
    # a round that never completes ends at simulations + 1 advances
    env._pool = _Recorder(rounds=10**9)
    gs = env.gumbel_search(ids, simulations=2, batch=2, seed=1)
    gs.run(lambda obs, mask, status: (np.zeros((6, 65), F), np.zeros(6, F)))
    assert [c[0] for c in env._pool.calls] == ["begin"] + ["advance"] * 3 + ["result", "end"]


def test_device_pool_checks_come_before_the_native_call():
    """A DevicePool without a native handle: whatever reaches the library fails on the missing attribute."""
    from envpool_amd.core.device_pool import DevicePool

    pool = object.__new__(DevicePool)
    pool.env_id_offset, pool.num_envs = 0, 4
    for bad in (0, 33, 2.5):
        with pytest.raises(ValueError, match="gumbel_begin: batch"):
            pool.gumbel_begin(np.zeros((4, 9), F), batch=bad)
        with pytest.raises(ValueError, match="gumbel_begin: batch"):
            pool.gumbel_begin_device(0, 0, 0, 0, batch=bad)
    pool._guided_k, pool._guided_policy, pool._gumbel_batch = 2, "gumbel", 4
    pool.guided_shape = lambda: (3, 3, 2, 9)
    for logits, values in ((np.zeros((2, 9), F), np.zeros(2, F)), (np.zeros((2, 3, 9), F), np.zeros((2, 3), F)),
                           (np.zeros((8, 9), F), np.zeros(4, F)), (np.full((2, 4, 9), np.inf, F), np.zeros((2, 4), F))):
        with pytest.raises(ValueError, match="gumbel_advance"):
            pool.gumbel_advance(logits, values)
    with pytest.raises(ValueError, match="reroot|Gumbel"):
        pool.guided_reroot(np.zeros(2, np.int32), 8)


def test_exported_symbols_and_header_agree():
    from envpool_amd.core import native

    header = open(os.path.join(ROOT, "include", "envpool_amd.h")).read()
    for name in ("epa_gumbel_begin_batch", "epa_gumbel_begin_batch_device"):
        assert name in native.EXPORTED_SYMBOLS and f"int {name}(" in header
    assert "#define EPA_GUMBEL_MAX_BATCH 32" in header
