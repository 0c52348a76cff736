"""PGX arena, CPU side: the contract header envpool_amd/csrc/pgx_arena.hip.h built for the host by g++
(tests/cpu_harness/pgx_arena_host.cpp) against the numpy restatement (pgx_arena_util.py), bit for bit; the argument
checks of the Python wrappers, which come before any native call; and the `Arena` session on a stand-in pool."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pgx_arena_util as AU
from envpool_amd.core import native
from envpool_amd.pgx.net import Net
from envpool_amd.python.envpool import Arena, ArenaStats
from test_pgx_selfplay_host import _StandIn as _SelfplayStandIn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"]
SRC = os.path.join(ROOT, "tests", "cpu_harness", "pgx_arena_host.cpp")
ROWS = [1, 63, 64, 65, 128, 129, 257]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pgx_arena") / "libpgxarenahost.so")
    subprocess.run(FLAGS + ["-shared", "-fPIC", SRC, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.ar_plan.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.ar_wave_map.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.ar_wave_map.restype = None
    L.ar_tally.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 4
    L.ar_tally.restype = None
    return L


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_net_of(lib):
    for e in range(8):
        for m in (0, 1):
            got = lib.ar_net_of(e, m)
            assert got == int(AU.net_of(e, m)) == (m ^ e) & 1
    # net A holds seat 0 of the even envs and seat 1 of the odd ones
    assert [lib.ar_net_of(e, e & 1) for e in range(8)] == [0] * 8
    assert lib.ar_net_of(1000003, 0) == 1 and lib.ar_net_of(1000003, 1) == 0


@pytest.mark.parametrize("rows", ROWS)
def test_plan_and_wave_mapping(lib, rows):
    patterns = AU.side_patterns(rows)
    assert {"all0", "all1", "alternating", "0then1", "1then0", "random", "n0=0", "n0=1"} <= set(patterns)
    assert f"n0={rows}" in patterns
    seen_n0 = set()
    for name, side in patterns.items():
        order = np.full(rows, -1, np.int32)
        n0 = lib.ar_plan(rows, _ptr(side), _ptr(order))
        want_order, want_n0 = AU.plan(side)
        assert n0 == want_n0 == int((side == 0).sum()), name
        assert np.array_equal(order, want_order), name
        seen_n0.add(n0)
        # stable: each side's rows ascend
        assert (np.diff(order[:n0]) > 0).all() and (np.diff(order[n0:]) > 0).all()
        assert not side[order[:n0]].any() and side[order[n0:]].all()
        waves = lib.ar_waves(rows)
        assert waves == AU.waves(rows) == -(-rows // 64) + 1
        wm = np.full((waves, 3), -1, np.int32)
        lib.ar_wave_map(rows, n0, _ptr(wm))
        assert np.array_equal(wm, AU.wave_map(rows, n0)), name
        # every row exactly once, no wave spans two nets, no wave beyond 64 entries or the plan's end
        count = np.zeros(rows, np.int64)
        for net, first, n in wm:
            assert 0 <= n <= 64 and (n == 0 or 0 <= first and first + n <= rows)
            mine = order[first:first + n]
            assert (side[mine] == net).all(), name
            count[mine] += 1
        assert (count == 1).all(), name
        used = int((wm[:, 2] > 0).sum())
        assert used == -(-n0 // 64) + -(-(rows - n0) // 64) <= waves
    for n0 in (0, 1, 63, 64, 65, rows):
        if n0 <= rows:
            assert n0 in seen_n0


def test_tally(lib):
    # both parities of e, a win for each seat and a draw, and rows that are not done
    done = np.array([1, 1, 1, 1, 1, 1, 0, 0], np.uint8)
    reward = np.array([[1, -1], [1, -1], [-1, 1], [-1, 1], [0, 0], [0, 0], [1, -1], [-1, 1]], np.float32)
    elapsed = np.array([5, 6, 7, 8, 9, 9, 100, 100], np.int32)
    for id0 in (0, 3):
        ids = id0 + np.arange(8)
        got = np.zeros(7, np.int64)
        lib.ar_tally(8, id0, _ptr(done), _ptr(reward), _ptr(elapsed), _ptr(got))
        assert np.array_equal(got, AU.tally(done, reward, elapsed, ids))
        # rows 0 .. 3: seat 0 wins in envs id0, id0 + 1, seat 1 in id0 + 2, id0 + 3: one win of each net per pair
        assert got.tolist() == [6, 2, 2, 2, 44, 2, 2]
        assert got[5] + got[6] + got[3] == got[0]
    # a single row: seat 0 wins in an even env (net A) and in an odd one (net B)
    for e, want in ((4, [1, 0]), (5, [0, 1])):
        got = np.zeros(7, np.int64)
        lib.ar_tally(1, e, _ptr(done[:1]), _ptr(reward[:1]), _ptr(elapsed[:1]), _ptr(got))
        assert got[5:].tolist() == want and got[:5].tolist() == [1, 1, 0, 0, 5]
    lib.ar_tally(1, 5, _ptr(done[:1]), _ptr(reward[:1]), _ptr(elapsed[:1]), _ptr(got))  # the counters add up
    assert got.tolist() == [2, 2, 0, 0, 10, 0, 2]


def test_sanitized_program(tmp_path):
    """The harness as a program of its own under the host sanitizers."""
    out = str(tmp_path / "pgx_arena_main")
    subprocess.run(FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DPGX_ARENA_MAIN",
                            SRC, "-o", out], check=True)
    run = subprocess.run([out], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr + run.stdout
    assert "bad 0 games 3 wins_a 1 wins_b 1" in run.stdout


def test_abi_names():
    header = open(os.path.join(ROOT, "include", "envpool_amd.h")).read()
    for name in ("epa_net_eval_pair", "epa_net_eval_pair_device", "epa_arena_begin", "epa_arena_stats"):
        assert name in native.EXPORTED_SYMBOLS and f"int {name}(" in header
    assert native.ARENA_MAX_ROWS == 1 << 20


def test_check_arena_refusals():
    a = Net.random((3, 3, 2), 9, 32, 0, seed=1)
    b = Net.random((3, 3, 2), 9, 128, 2, seed=2)  # D and L may differ
    o = native.check_arena(a, b)
    assert (o.policy, o.simulations, o.noise, o.record, o.batch) == (0, 32, 1, 0, 0)  # record is off by default
    assert native.check_arena(a, b, record=True, policy="puct", sample_plies=4, width=2).record == 1
    with pytest.raises(ValueError, match="arena: net_a must be an envpool_amd.pgx.net.Net"):
        native.check_arena(lambda *x: None, b)
    with pytest.raises(ValueError, match="arena: net_b must be an envpool_amd.pgx.net.Net"):
        native.check_arena(a, None)
    with pytest.raises(ValueError, match=r"arena: net_a has F = 18, A = 9 and net_b F = 18, A = 7: the two nets must"):
        native.check_arena(a, Net.random((3, 3, 2), 7, 32, 0))
    with pytest.raises(ValueError, match=r"arena: net_a has F = 18, A = 9 and net_b F = 27, A = 9"):
        native.check_arena(a, Net.random((3, 3, 3), 9, 32, 0))
    # every refusal of selfplay's options applies
    for kw, msg in ((dict(policy="uct"), "selfplay: policy = 'uct'"),
                    (dict(policy="gumbel", width=2), r"selfplay: \['width'\] are arguments of policy='puct'"),
                    (dict(policy="puct", batch=4), r"selfplay: \['batch'\] are arguments of policy='gumbel'"),
                    (dict(seed=-1), "selfplay: seed = -1"), (dict(record=1), "selfplay: record = 1"),
                    (dict(batch=33), "gumbel_begin: batch = 33 must be 1 .. 32"),
                    (dict(simulations=0), "gumbel_begin: simulations = 0")):
        with pytest.raises(ValueError, match=msg):
            native.check_arena(a, b, **kw)
    # the side bytes of the direct host form
    s = native.check_arena_side([0, 1, 1], 3)
    assert s.dtype == np.uint8 and s.tolist() == [0, 1, 1]
    assert native.check_arena_side(np.array([True, False]), 2).tolist() == [1, 0]
    for side, rows, msg in (([0, 2, 1], 3, "net_eval_pair: side must be 0 .net_a. or 1 .net_b. in every row"),
                            ([0, -1], 2, "net_eval_pair: side must be 0"), ([0.0, 1.0], 2, "net_eval_pair: side must"),
                            ([0, 1], 3, r"net_eval_pair: side has shape \(2,\) for 3 rows"),
                            ([[0, 1]], 2, r"net_eval_pair: side has shape \(1, 2\) for 2 rows")):
        with pytest.raises(ValueError, match=msg):
            native.check_arena_side(side, rows)


class _StandIn(_SelfplayStandIn):
    """The self-play stand-in with the arena's calls: the plies are the driver's (`selfplay_run`)."""

    def arena_begin(self, net_a, net_b, **options):
        native.check_arena(net_a, net_b, **options)
        self.net, self.options = net_a, dict(options)
        self.calls.append(("arena_begin", net_a, net_b, dict(options)))

    def arena_run(self, plies, wait=True):
        self.selfplay_run(plies, wait)

    def arena_stats(self):
        self.calls.append(("arena_stats",))
        return np.array([3, 1, 1, 1, 20, 2, 0, self.t], np.int64)

    def arena_end(self):
        self.calls.append(("arena_end",))


def test_arena_session_on_a_stand_in_pool():
    a, b = Net.random((1, 1, 2), 7, 32, 0, seed=1), Net.random((1, 1, 2), 7, 64, 1, seed=2)
    pool = _StandIn()
    arena = Arena(pool, a, b, dict(policy="gumbel", simulations=8, batch=4, seed=3, record=False))
    assert pool.calls[0][:3] == ("arena_begin", a, b) and pool.calls[0][3]["batch"] == 4
    stats = arena.run(3)
    assert stats == ArenaStats(3, 1, 1, 1, 20, 2, 0, 3) and isinstance(stats.wins_a, int)
    assert ArenaStats._fields == ("games", "wins0", "wins1", "draws", "plies", "wins_a", "wins_b", "t")
    assert arena.run(2, wait=False) is None
    assert arena.stats().t == 5
    names = [c[0] for c in pool.calls]
    assert [n for n in names if n.startswith(("arena", "selfplay"))] == [
        "arena_begin", "selfplay_run", "arena_stats", "selfplay_run", "arena_stats"]
    assert ("selfplay_run", 3, True) in pool.calls and ("selfplay_run", 2, False) in pool.calls
    per_ply = ["begin"] + ["advance"] * 9 + ["result", "end"]
    assert [n for n in names if not n.startswith(("arena", "selfplay"))] == per_ply * 5
    with pytest.raises(ValueError, match="selfplay_run: plies = 0 must be at least 1"):
        arena.run(0)
    arena.close()
    arena.close()  # (closing twice is fine)
    assert [c[0] for c in pool.calls].count("arena_end") == 1
    with pytest.raises(ValueError, match="arena: the arena is closed"):
        arena.run(1)
    with pytest.raises(ValueError, match="arena: net_a has F = 2, A = 7 and net_b F = 2, A = 9"):
        Arena(_StandIn(), a, Net.random((1, 1, 2), 9, 32, 0), {})
    with pytest.raises(ValueError, match="gumbel_begin: batch = 40"):
        Arena(_StandIn(), a, b, dict(batch=40))
