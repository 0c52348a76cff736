"""PGX exact solver with transposition tables (solve table_bits=), CPU side: the solver of
envpool_amd/csrc/pgx_solve.hip.h with every lane's private table, built for the host by g++
(tests/cpu_harness/pgx_solve_table_host.cpp, which walks a wave's lanes as loops), against the brute-force minimax in value, q, action and status; against the table-less harness
where the trees are too large for the brute force and, at table_bits = 0, in all five outputs; the key of an entry field
by field; the positions saved; rows that are given up without a table and solved with one; determinism; and the
argument checks of the Python wrappers, which come before any native call.

The positions are those of test_pgx_solve_host.py (70 envs per set, env 33 marked over, the hand-made wins and losses,
late Othello) and ConnectFour 24 plies in to the end of the game (pgx_solve_table_util.py)."""
import ctypes

import numpy as np
import pytest

from pgx_solve_table_util import (DEEP_ENVS, GIVE_BITS, GIVE_ENVS, GIVE_NODES, HEX_DEEP_ROWS, MAX_TABLE_BITS, NAMES,
                                  build_libs, deep_connect_four, early, empty_tictactoe, key_test, late_othello,
                                  table_solve)
from pgx_solve_util import BIG, DEPTHS, GAMES, brute_solve, hand_made, host_solve

BITS = (2, 6, 10)  # 2: four entries per lane, every store replaces and unrelated positions share slots


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    return build_libs(tmp_path_factory.mktemp("pgx_solve_table"))


@pytest.fixture(scope="module")
def deep(libs):
    """The DEEP rows of ConnectFour and their table-less solve."""
    hid, done = deep_connect_four(libs, DEEP_ENVS)
    return hid, done, host_solve(libs["solve_host"], "ConnectFour", hid, done, 0)[0]


@pytest.fixture(scope="module")
def late(libs):
    hid, done = late_othello(libs)
    return hid, done, host_solve(libs["solve_host"], "Othello", hid, done, 0)[0]


def same(got, want, what, names=NAMES):
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert np.array_equal(g, w), (what, name, np.flatnonzero((g != w).reshape(len(g), -1).any(1)))


def sets(libs, fam):
    """[(hidden, done, depth)]: the early positions at DEPTHS, the hand-made positions at their depth and one less."""
    out = []
    for hid, done in early(libs, fam):
        for depth in DEPTHS[fam]:
            rows = slice(0, HEX_DEEP_ROWS) if (fam, depth) == ("Hex", 3) else slice(None)
            out.append((hid[rows], done[rows], depth))
    for words, depth, _, _ in hand_made(fam):
        out += [(words[None], np.zeros(1, np.uint8), depth), (words[None], np.zeros(1, np.uint8), depth - 1)]
    return out


# ---- 1. values ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", GAMES)
def test_values_equal_the_brute_force(libs, fam):
    seen = set()
    for hid, done, depth in sets(libs, fam):
        want = brute_solve(libs["solve_brute"], fam, hid, done, depth)[0]
        for bits in BITS:
            got, broken = table_solve(libs["solve_table_host"], fam, hid, done, depth, bits)
            same(got[:4], want, (fam, depth, bits), NAMES[:4])
            assert not broken.any() and (got[4][got[3] == 0] > 1).all() and (got[4][got[3] == 2] == 0).all()
        seen |= set(want[0][want[3] == 0].tolist())
    assert seen == {-1, 0, 1}


def test_late_othello_equals_the_brute_force(libs, late):
    hid, done, _ = late
    want = brute_solve(libs["solve_brute"], "Othello", hid, done, 0)[0]
    for bits in BITS:
        same(table_solve(libs["solve_table_host"], "Othello", hid, done, 0, bits)[0][:4], want, bits, NAMES[:4])


def test_deep_connect_four_equals_the_table_less_harness(libs, deep):
    hid, done, want = deep
    assert (want[3] == 0).all() and set(want[0].tolist()) == {-1, 0, 1}
    for bits in BITS:
        got, broken = table_solve(libs["solve_table_host"], "ConnectFour", hid, done, 0, bits)
        same(got[:4], want[:4], bits, NAMES[:4])
        assert not broken.any()


# ---- 2. table_bits = 0 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", GAMES)
def test_no_table_is_the_table_less_harness(libs, fam, late):
    cases = sets(libs, fam) + ([(late[0], late[1], 0)] if fam == "Othello" else [])
    for hid, done, depth in cases:
        for max_nodes in (BIG, 3000):
            got, broken = table_solve(libs["solve_table_host"], fam, hid, done, depth, 0, max_nodes)
            want, wbroken = host_solve(libs["solve_host"], fam, hid, done, depth, max_nodes)
            same(got, want, (fam, depth, max_nodes))
            assert np.array_equal(broken, wbroken)


# ---- 3. the key ---------------------------------------------------------------------------------------------------
def _with_stone(fam, words, which):
    """`words` with one more stone of set a or b on the first empty cell."""
    color_board = fam in ("TicTacToe", "ConnectFour")
    cells = len(words) - (3 if fam == "Othello" else 2)
    empty, stone = (-1, {"a": 0, "b": 1}[which]) if color_board else (0, {"a": 1, "b": -1}[which])
    out = words.copy()
    out[np.flatnonzero(words[:cells] == empty)[0]] = stone
    return out


def _with_word(words, index, value):
    out = words.copy()
    out[index] = value
    return out


@pytest.mark.parametrize("fam", GAMES)
def test_a_hit_needs_every_field_that_matters(libs, fam):
    """One entry (every key has its slot): a stored position is found with its bounds; a position that differs in a, b,
    the plies left, or the game's flag -- TicTacToe / ConnectFour turn, Hex turn by class, Othello passed -- is not.
    cp, Othello's turn and a Hex turn of the same class do not matter (pgx_solve.hip.h argues why), and hit."""
    lib = libs["solve_table_host"]
    base = early(libs, fam)[0][0][0].astype(np.int32)
    cells = len(base) - (3 if fam == "Othello" else 2)
    turn, cp = cells, cells + 1
    if fam == "Hex":
        base = _with_word(base, turn, 3)
    for lo, hi in ((-1, -1), (-1, 0), (-1, 1), (0, 0), (0, 1), (1, 1)):
        assert key_test(lib, fam, base, base, (5, 5), lo, hi) == (lo, hi)
    assert key_test(lib, fam, base, base, (2, 2), 0, 1) == (0, 1)
    assert key_test(lib, fam, base, base, (128, 128), 0, 1) == (0, 1)
    miss = [(_with_stone(fam, base, "a"), (5, 5)), (_with_stone(fam, base, "b"), (5, 5)),
            (base, (5, 4)), (base, (5, 6)), (base, (5, 128)), (base, (69, 5))]
    hit = [_with_word(base, cp, 1 - base[cp])]
    if fam == "Hex":
        miss += [(_with_word(base, turn, t), (5, 5)) for t in (0, 1, 2, 4)]  # 3 against 1: the swap; against even
        hit += [_with_word(base, turn, 5), _with_word(base, turn, 121)]
        for t, other in ((0, 2), (1, 3), (2, 0), (2, 3)):
            assert key_test(lib, fam, _with_word(base, turn, t), _with_word(base, turn, other), (5, 5), 0, 0) is None
        assert key_test(lib, fam, _with_word(base, turn, 2), _with_word(base, turn, 4), (5, 5), 0, 0) == (0, 0)
    elif fam == "Othello":
        miss.append((_with_word(base, cells + 2, 1 - base[cells + 2]), (5, 5)))
        hit.append(_with_word(base, turn, 1 - base[turn]))
    else:
        miss.append((_with_word(base, turn, 1 - base[turn]), (5, 5)))
    for probed, plies in miss:
        assert key_test(lib, fam, base, probed, plies, 0, 0) is None, (fam, np.flatnonzero(probed != base), plies)
    for probed in hit:
        assert key_test(lib, fam, base, probed, (5, 5), -1, 0) == (-1, 0), (fam, np.flatnonzero(probed != base))
    assert lib.pgx_solve_table_floor() >= 1 and lib.pgx_solve_table_max_bits() == MAX_TABLE_BITS
    lib.pgx_solve_table_bytes.restype = ctypes.c_longlong
    assert [lib.pgx_solve_table_bytes(b) for b in (0, 1, 16)] == [0, 64 * 2 * 32, 64 * 65536 * 32]


# ---- 4. total positions -------------------------------------------------------------------------------------------
def test_a_table_visits_fewer_positions(libs, deep, late):
    """Summed `nodes` at table_bits = 10 strictly below the table-less sum (the counts: pgx_solve_table_util.py)."""
    lib = libs["solve_table_host"]
    hid, done = empty_tictactoe(libs)
    plain = host_solve(libs["solve_host"], "TicTacToe", hid, done, 0)[0]
    cases = [("TicTacToe", hid, done, plain), ("ConnectFour",) + deep, ("Othello",) + late]
    for fam, hid, done, plain in cases:
        got = table_solve(lib, fam, hid, done, 0, 10)[0]
        same(got[:4], plain[:4], fam, NAMES[:4])
        print(fam, int(plain[4].sum()), "->", int(got[4].sum()))
        assert 0 < got[4].sum() < plain[4].sum(), fam


# ---- 5. given up becomes solved -----------------------------------------------------------------------------------
def test_given_up_without_a_table_is_solved_with_one(libs):
    hid, done = deep_connect_four(libs, GIVE_ENVS)
    assert len(hid) >= 4
    plain = host_solve(libs["solve_host"], "ConnectFour", hid, done, 0, GIVE_NODES)[0]
    assert (plain[3] == 1).all() and (plain[0] == 0).all() and (plain[2] == -1).all() and (plain[1] == -128).all()
    got = table_solve(libs["solve_table_host"], "ConnectFour", hid, done, 0, GIVE_BITS, GIVE_NODES)[0]
    want = host_solve(libs["solve_host"], "ConnectFour", hid, done, 0, BIG)[0]
    assert (got[3] == 0).all() and (want[3] == 0).all()
    same(got[:4], want[:4], "values", NAMES[:4])
    print("table-less", want[4].tolist(), "table_bits", GIVE_BITS, got[4].tolist())
    # away from max_nodes on both sides, which is looked at between rounds only
    assert (want[4] > 4 * GIVE_NODES).all() and (got[4] < GIVE_NODES // 2).all()


# ---- 6. determinism -----------------------------------------------------------------------------------------------
def test_the_bytes_repeat_and_rows_do_not_depend_on_each_other(libs, late, deep):
    lib = libs["solve_table_host"]
    for fam, (hid, done, _), bits, max_nodes in (("Othello", late, 6, BIG), ("Othello", late, 3, 8000),
                                                 ("ConnectFour", deep, 8, 300_000)):
        first = table_solve(lib, fam, hid, done, 0, bits, max_nodes)[0]
        again = table_solve(lib, fam, hid, done, 0, bits, max_nodes)[0]
        for g, w in zip(again, first):
            assert g.tobytes() == w.tobytes()
        if max_nodes != BIG:
            assert (first[3] == 1).any() and (first[3] == 0).any()
        n = len(hid)
        order = np.r_[np.random.default_rng(4).permutation(n), [3, 3, 0]]  # shuffled, then repeated
        same(table_solve(lib, fam, hid[order], done[order], 0, bits, max_nodes)[0], [w[order] for w in first], fam)


# ---- 7. wrappers --------------------------------------------------------------------------------------------------
BAD_BITS = [-1, 17, 1.5, True, 2**40]


def test_check_solve_table_bits():
    from envpool_amd.core import native

    assert native.SOLVE_MAX_TABLE_BITS == MAX_TABLE_BITS
    assert native.check_solve([[3, 1], [2, 2]], 0, 1 << 20).tolist() == [3, 1, 2, 2]  # optional: today's callers
    for bits in (0, 1, 16, np.int64(8)):
        assert native.check_solve([0, 0], 4, 1, bits).dtype == np.int32
        assert native.check_solve([0], 4, 1, table_bits=bits).tolist() == [0]
    for bits in BAD_BITS:
        with pytest.raises(ValueError, match=r"solve: table_bits = .* must be in 0 \.\. 16"):
            native.check_solve([0], 0, 1 << 20, bits)
    with pytest.raises(ValueError, match="solve: table_bits = 17 must be in 0 .. 16"):
        native.check_solve([0], 0, 1 << 20, 17)
    with pytest.raises(ValueError, match="depth"):  # the earlier checks come first
        native.check_solve([0], -1, 1 << 20, 17)
    names = {"epa_solve", "epa_solve_device", "epa_solve_table", "epa_solve_table_device"}
    assert names <= set(native.EXPORTED_SYMBOLS) and len(set(native.EXPORTED_SYMBOLS)) == len(native.EXPORTED_SYMBOLS)


class _Recorder:
    def __init__(self):
        self.calls = []

    def solve(self, env_ids, depth, max_nodes, table_bits=0):
        self.calls.append((np.asarray(env_ids), depth, max_nodes, table_bits))
        k = len(env_ids)
        return (np.zeros(k, np.int8), np.zeros((k, 7), np.int8), np.zeros(k, np.int32), np.zeros(k, np.uint8),
                np.zeros(k, np.int64))


def test_wrapper_checks_come_before_the_native_call():
    from envpool_amd.core.binding import _ShardedPools
    from envpool_amd.core.device_pool import DevicePool
    from envpool_amd.pgx import ConnectFourGymnasiumEnvPool
    from envpool_amd.torch_interop import solve_device

    env = object.__new__(ConnectFourGymnasiumEnvPool)
    env._pool = _Recorder()
    ids = np.array([2, 0, 1], np.int32)
    out = env.solve(ids, depth=6, max_nodes=1000, table_bits=9)
    assert out._fields == NAMES and out.q.shape == (3, 7)
    env.solve(ids, 0, 5)
    assert [c[1:] for c in env._pool.calls] == [(6, 1000, 9), (0, 5, 0)]
    for bits in BAD_BITS:
        with pytest.raises(ValueError, match=r"solve: table_bits = .* must be in 0 \.\. 16"):
            env.solve(ids, table_bits=bits)
    assert len(env._pool.calls) == 2
    # the layers below: refused before the library is touched (these pools have none)
    pool = object.__new__(DevicePool)
    sharded = object.__new__(_ShardedPools)
    for bits in BAD_BITS:
        with pytest.raises(ValueError, match="solve: table_bits"):
            pool.solve(ids, 0, 1 << 20, bits)
        with pytest.raises(ValueError, match="solve: table_bits"):
            pool.solve_device(0, 0, 0, 0, 0, ids, table_bits=bits)
        with pytest.raises(ValueError, match="solve: table_bits"):
            sharded.solve(ids, table_bits=bits)
        with pytest.raises(ValueError, match="solve: table_bits"):
            solve_device(pool, ids, table_bits=bits)


def test_a_family_without_solve_raises_with_the_keyword():
    from envpool_amd.classic_control import CartPoleGymnasiumEnvPool

    env = object.__new__(CartPoleGymnasiumEnvPool)
    env._pool = object()
    with pytest.raises(RuntimeError, match="solve not implemented for this environment"):
        env._solve(np.zeros(1, np.int32), 0, 1, 8)
