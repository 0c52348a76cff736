"""PGX self-play driver, CPU side: the contract header envpool_amd/csrc/pgx_selfplay.hip.h built for the host by g++
(tests/cpu_harness/pgx_selfplay_host.cpp) against the numpy restatement (pgx_selfplay_util.py), bit for bit; the error
of the noise against float64; the argument checks of the Python wrappers, which come before any native call; and the
`Selfplay` session on a stand-in pool."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pgx_selfplay_util as U
from envpool_amd.core import native
from envpool_amd.pgx.net import Net
from envpool_amd.python.envpool import GumbelSearch, Selfplay, Stats
from test_pgx_net_host import _StandIn as _NetStandIn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"]  # no fast-math, no contraction
SRC = os.path.join(ROOT, "tests", "cpu_harness", "pgx_selfplay_host.cpp")
N23 = 1 << 23
F = np.float32


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pgx_selfplay") / "libpgxselfplayhost.so")
    subprocess.run(FLAGS + ["-shared", "-fPIC", SRC, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.sp_key.restype = ctypes.c_uint64
    L.sp_key.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_uint32]
    L.sp_sample_at.restype = ctypes.c_uint32
    L.sp_sample_at.argtypes = [ctypes.c_uint64, ctypes.c_uint32]
    L.sp_noise_rows.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int,
                                ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.sp_noise_of.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.sp_pick_sampled.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32]
    for f in (L.sp_gumbel_log, L.sp_noise_of, L.sp_noise_rows, L.sp_puct, L.sp_gumbel_actions, L.sp_tally):
        f.restype = None
    return L


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


@pytest.fixture(scope="module")
def all_noise(lib):
    """u and g of all 2^23 values of n, from the header."""
    u, g = np.empty(N23, F), np.empty(N23, F)
    lib.sp_noise_of(0, N23, _ptr(u), _ptr(g))
    return u, g


def test_gumbel_log_bit_for_bit(lib, all_noise):
    u, g = all_noise
    n = np.arange(N23, dtype=np.uint32)
    ru = U.uniform_of(n)
    assert np.array_equal(bits(u), bits(ru))
    assert u.min() > 0 and u.max() < 1  # strictly inside: 24 bits would round the top value to 1.0
    assert float(F((F(2 ** 24 - 1) + F(0.5)) * F(2.0 ** -24))) == 1.0
    assert np.array_equal(bits(g), bits(U.noise_of(ru)))
    # GumbelLog itself on all 2^23 uniforms, and on their negated logarithms (the noise's second argument)
    for x in (u, -U.gumbel_log(ru)):
        x = np.ascontiguousarray(x, F)
        out = np.empty(N23, F)
        lib.sp_gumbel_log(N23, _ptr(x), _ptr(out))
        assert np.array_equal(bits(out), bits(U.gumbel_log(x)))
    # powers of two, their neighbours, FLT_MIN and 17.0
    p2 = np.ldexp(F(1.0), np.arange(-126, 128)).astype(F)
    x = np.concatenate([p2, np.nextafter(p2, F(0)), np.nextafter(p2[:-1], F(np.inf)),
                        np.array([np.finfo(F).tiny, 17.0, 0.70710678, 0.7071067, 0.7071069, 1.0, 3.0], F)]).astype(F)
    x = np.ascontiguousarray(x[(x >= np.finfo(F).tiny) & np.isfinite(x)])
    out = np.empty(len(x), F)
    lib.sp_gumbel_log(len(x), _ptr(x), _ptr(out))
    ref = U.gumbel_log(x)
    assert np.array_equal(bits(out), bits(ref))
    assert np.abs(ref.astype(np.float64) - np.log(x.astype(np.float64))).max() < 2e-5 * 90  # a logarithm, all the way
    assert out[np.flatnonzero(x == F(1.0))[0]] == 0.0


def test_noise_error_against_float64(all_noise):
    """All 2^23 values: |g - (-log(-log(u)))| in float64 stays below 2e-6 (the sampled figure with a 3.5x margin), g is
    finite and lies in the stated range."""
    u, g = all_noise
    u64 = u.astype(np.float64)
    err = np.abs(g.astype(np.float64) + np.log(-np.log(u64)))
    print(f"exhaustive max |g - float64| = {err.max():.3e} at n = {int(err.argmax())}; g in {g.min():.4f} .. "
          f"{g.max():.4f}; mean {g.astype(np.float64).mean():.4f} var {g.astype(np.float64).var():.4f}")
    assert np.isfinite(g).all()
    assert err.max() < 2e-6
    assert -2.82 < g.min() < -2.80 and 16.6 < g.max() < 16.7
    assert abs(g.astype(np.float64).mean() - 0.5772) < 1e-3 and abs(g.astype(np.float64).var() - np.pi ** 2 / 6) < 5e-3


@pytest.mark.parametrize("actions", [9, 7, 122, 65])
def test_noise_rows(lib, actions):
    """Rows of ids with an offset, several plies and seeds; noise off gives zeros."""
    k, id0 = 37, 1000003
    ids = np.arange(id0, id0 + k)
    for seed, t in ((0, 0), (12345678901234567890, 7), (2 ** 64 - 1, 2 ** 32 - 1)):
        u, g = np.empty((k, actions), F), np.empty((k, actions), F)
        lib.sp_noise_rows(seed, id0, k, t, actions, 1, _ptr(u), _ptr(g))
        keys = U.key(seed, ids, t)
        assert [lib.sp_key(seed, int(e), t) for e in ids[:5]] == [int(x) for x in keys[:5]]
        assert np.array_equal(bits(u), bits(U.uniform(keys, actions)))
        assert np.array_equal(bits(g), bits(U.noise_rows(seed, ids, t, actions)))
        lib.sp_noise_rows(seed, id0, k, t, actions, 0, _ptr(u), _ptr(g))
        assert not g.any() and not U.noise_rows(seed, ids, t, actions, noise=False).any()
    a = U.noise_rows(1, ids, 0, actions)
    assert not np.array_equal(a, U.noise_rows(2, ids, 0, actions))
    assert not np.array_equal(a, U.noise_rows(1, ids, 1, actions))
    assert not np.array_equal(a[0], a[1])


def host_puct(lib, visits, result_action, elapsed, sample_plies, keys):
    visits = np.ascontiguousarray(visits, np.int32)
    k, a = visits.shape
    ra, el = np.ascontiguousarray(result_action, np.int32), np.ascontiguousarray(elapsed, np.int32)
    keys = np.ascontiguousarray(keys, np.uint64)
    action, target = np.full(k, -7, np.int32), np.full((k, a), -1, F)
    lib.sp_puct(k, a, _ptr(visits), _ptr(ra), _ptr(el), sample_plies, _ptr(keys), _ptr(action), _ptr(target))
    return action, target


def test_puct_picks_hand_made(lib):
    a = 9
    one = np.zeros(a, np.int32)
    one[5] = 8                                  # all visits on one action
    ties = np.array([0, 3, 3, 0, 3, 0, 0, 0, 0], np.int32)
    mixed = np.array([2, 0, 1, 0, 0, 4, 0, 0, 1], np.int32)
    none = np.zeros(a, np.int32)
    # r at 0, at V - 1 and at every prefix boundary
    for row in (one, ties, mixed):
        prefix, V = np.cumsum(row), int(row.sum())
        for r in range(V):
            want = int(np.flatnonzero(prefix > r)[0])
            assert lib.sp_pick_sampled(_ptr(row), a, r) == want
            assert row[want] > 0
        assert lib.sp_pick_sampled(_ptr(row), a, 0) == int(np.flatnonzero(row)[0])
        assert lib.sp_pick_sampled(_ptr(row), a, V - 1) == int(np.flatnonzero(row)[-1])
        for b in np.unique(prefix[(prefix > 0) & (prefix < V)]):  # one below and at a boundary: the two sides of it
            assert lib.sp_pick_sampled(_ptr(row), a, int(b) - 1) < lib.sp_pick_sampled(_ptr(row), a, int(b))
    assert lib.sp_pick_greedy(_ptr(one), a) == 5 and lib.sp_pick_greedy(_ptr(ties), a) == 1
    assert lib.sp_pick_greedy(_ptr(mixed), a) == 5
    # whole rows through the rule, against the restatement; keys chosen so that r takes 0 and V - 1
    rows, ra, el, keys = [], [], [], []
    for row in (one, ties, mixed):
        V = int(row.sum())
        seen = {}
        for key in range(4000):
            r = lib.sp_sample_at(key, V)
            assert 0 <= r < V and r == int(U.sample_at(np.array([key], np.uint64), np.array([V]))[0])
            seen.setdefault(r, key)
        assert 0 in seen and V - 1 in seen
        for r, key in seen.items():
            for elapsed in (0, 3, 4, 5):       # sample_plies = 4: both sides of the elapsed step
                rows.append(row), ra.append(2), el.append(elapsed), keys.append(key)
    rows.append(none), ra.append(0), el.append(0), keys.append(1)      # V = 0
    rows.append(mixed), ra.append(-1), el.append(0), keys.append(1)    # the root was over
    action, target = host_puct(lib, np.array(rows), ra, el, 4, keys)
    want_a, want_t = U.puct_move(np.array(rows), np.array(ra), np.array(el), 4, np.array(keys, np.uint64))
    assert np.array_equal(action, want_a) and np.array_equal(bits(target), bits(want_t))
    assert action[-1] == 0 and action[-2] == 0 and not target[-2:].any()
    el = np.array(el)
    greedy = el[:-2] >= 4
    assert (action[:-2][greedy] == np.array([lib.sp_pick_greedy(_ptr(r), a) for r in rows[:-2]])[greedy]).all()
    assert len(set(action[:-2][~greedy].tolist())) > 3  # sampling does move
    assert np.allclose(target[:-2].sum(axis=1), 1.0, atol=1e-6)
    # random rows of every game's width
    rng = np.random.default_rng(0)
    for a in (7, 9, 65, 122):
        k = 200
        v = rng.integers(0, 6, size=(k, a)) * (rng.random((k, a)) < 0.3)
        ra_, el_ = rng.integers(-1, a, size=k), rng.integers(0, 8, size=k)
        keys_ = rng.integers(0, 2 ** 63, size=k).astype(np.uint64)
        got = host_puct(lib, v, ra_, el_, 4, keys_)
        want = U.puct_move(v, ra_, el_, 4, keys_)
        assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))


def test_gumbel_move_and_tally(lib):
    ra = np.array([-1, 0, 5, -1, 64], np.int32)
    out = np.empty(5, np.int32)
    lib.sp_gumbel_actions(5, _ptr(ra), _ptr(out))
    w = np.arange(10, dtype=F).reshape(5, 2)
    a, t = U.gumbel_move(ra, w)
    assert np.array_equal(out, a) and out.tolist() == [0, 0, 5, 0, 64] and t is not None and np.array_equal(t, w)
    done = np.array([1, 0, 1, 1, 1, 0, 1], np.uint8)
    reward = np.array([[1, -1], [1, -1], [-1, 1], [0, 0], [1, 1], [0, 0], [-1, -1]], F)
    elapsed = np.array([5, 100, 9, 9, 7, 100, 1], np.int32)
    got = np.zeros(5, np.int64)
    lib.sp_tally(7, _ptr(done), _ptr(reward), _ptr(elapsed), _ptr(got))
    assert got.tolist() == [5, 2, 2, 1, 31]
    assert np.array_equal(got, U.tally(done, reward, elapsed))
    lib.sp_tally(7, _ptr(done), _ptr(reward), _ptr(elapsed), _ptr(got))  # the counters add up
    assert got.tolist() == [10, 4, 4, 2, 62]


def test_sanitized_program(tmp_path):
    """The harness as a program of its own under the host sanitizers."""
    out = str(tmp_path / "pgx_selfplay_main")
    subprocess.run(FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DPGX_SELFPLAY_MAIN",
                            SRC, "-o", out], check=True)
    run = subprocess.run([out], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr + run.stdout
    assert "games 3" in run.stdout


def test_abi_names_and_struct():
    header = open(os.path.join(ROOT, "include", "envpool_amd.h")).read()
    for name in ("epa_selfplay_begin", "epa_selfplay_run", "epa_selfplay_run_device", "epa_selfplay_stats",
                 "epa_selfplay_end"):
        assert name in native.EXPORTED_SYMBOLS and f"int {name}(" in header
    # the ctypes struct has the header's fields in the header's order
    body = header[header.index("typedef struct epa_selfplay_options {"):header.index("} epa_selfplay_options;")]
    fields = [line.split(";")[0].split()[-1] for line in body.splitlines()[1:] if ";" in line]
    assert fields == [f[0] for f in native.SelfplayOptions._fields_]
    assert ctypes.sizeof(native.SelfplayOptions) == 72


def test_check_selfplay_refusals():
    o = native.check_selfplay()
    assert (o.policy, o.simulations, o.max_considered, o.batch, o.noise, o.record) == (0, 32, 16, 0, 1, 1)
    assert (o.width, o.tactics, o.prove, o.sample_plies, o.tactics_nodes, o.c_puct) == (0, 0, 0, 0, 0, 0.0)
    o = native.check_selfplay(policy="gumbel", simulations=8, max_considered=4, batch=4, seed=2 ** 64 - 1, noise=False,
                              record=False)
    assert (o.batch, o.seed, o.noise, o.record, o.max_considered) == (4, 2 ** 64 - 1, 0, 0, 4)
    o = native.check_selfplay(policy="puct", simulations=8, width=2, sample_plies=4, tactics=2, prove=True, c_puct=2.0)
    assert (o.policy, o.width, o.sample_plies, o.tactics, o.prove, o.c_puct, o.batch) == (1, 2, 4, 2, 1, 2.0, 0)
    assert o.tactics_nodes == native.GUIDED_TACTICS_NODES
    assert (o.max_considered, o.noise, o.c_visit, o.c_scale) == (0, 0, 0.0, 0.0)  # the Gumbel fields stay 0
    assert native.check_selfplay(policy="puct", width=1).width == 0  # 1 is the plain session
    bad = [
        (dict(policy="uct"), "selfplay: policy = 'uct' must be 'puct' or 'gumbel'"),
        (dict(policy="gumbel", width=2), r"selfplay: \['width'\] are arguments of policy='puct'"),
        (dict(policy="gumbel", tactics=2, prove=True), r"selfplay: \['prove', 'tactics'\] are arguments of policy='puct'"),
        (dict(policy="gumbel", sample_plies=4), r"selfplay: \['sample_plies'\] are arguments of policy='puct'"),
        (dict(policy="gumbel", c_puct=1.0), r"selfplay: \['c_puct'\] are arguments of policy='puct'"),
        (dict(policy="puct", batch=4), r"selfplay: \['batch'\] are arguments of policy='gumbel'"),
        (dict(policy="puct", max_considered=4, noise=False),
         r"selfplay: \['max_considered', 'noise'\] are arguments of policy='gumbel'"),
        (dict(seed=-1), "selfplay: seed = -1 must be an integer"),
        (dict(seed=2 ** 64), "selfplay: seed ="),
        (dict(seed=1.5), "selfplay: seed ="),
        (dict(record=1), "selfplay: record = 1 must be True or False"),
        (dict(noise=1), "selfplay: noise = 1 must be True or False"),
        (dict(simulations=0), "gumbel_begin: simulations = 0 must be 1 .. 4096"),
        (dict(simulations=4097), "gumbel_begin: simulations = 4097"),
        (dict(max_considered=0), "gumbel_begin: max_considered = 0 must be at least 1"),
        (dict(c_visit=-1.0), "gumbel_begin: c_visit = -1.0 must be finite and >= 0"),
        (dict(c_scale=float("nan")), "gumbel_begin: c_scale"),
        (dict(batch=33), "gumbel_begin: batch = 33 must be 1 .. 32"),
        (dict(batch=0), "gumbel_begin: batch = 0 must be 1 .. 32"),
        (dict(policy="puct", simulations=0), "guided_begin: simulations = 0 must be 1 .. 4096"),
        (dict(policy="puct", c_puct=-1.0), "guided_begin: c_puct = -1.0 must be finite and >= 0"),
        (dict(policy="puct", width=33), "guided_begin: width = 33 must be 1 .. 32"),
        (dict(policy="puct", tactics=17), "guided_begin: tactics = 17 must be 0 .. 16"),
        (dict(policy="puct", tactics=2, tactics_nodes=0), "guided_begin: tactics_nodes = 0 must be 1 .."),
        (dict(policy="puct", prove=1), "guided_begin: prove = 1 must be True or False"),
        (dict(policy="puct", sample_plies=-1), "selfplay: sample_plies = -1 must be an integer >= 0"),
        (dict(policy="puct", sample_plies=1.5), "selfplay: sample_plies = 1.5"),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            native.check_selfplay(**kw)
    assert native.check_selfplay_plies(np.int64(3)) == 3
    for plies in (0, -1, True, 1.5):
        with pytest.raises(ValueError, match="selfplay_run: plies"):
            native.check_selfplay_plies(plies)


class _StandIn(_NetStandIn):
    """The stand-in pool of the `run(net)` tests with the driver's calls: `selfplay_run` makes, per ply, the session
    calls the host-driven loop makes on it -- begin, the round through `net_run`, result, end."""

    def __init__(self, k=3, a=7, simulations=8):
        super().__init__(k, a, simulations)
        self.t, self.net, self.options = 0, None, None

    def selfplay_begin(self, net, **options):
        native.check_selfplay(**options)
        self.net, self.options = net, dict(options)
        self.calls.append(("selfplay_begin", net, dict(options)))

    def selfplay_run(self, plies, wait=True):
        self.calls.append(("selfplay_run", plies, wait))
        ids = np.arange(self.k, dtype=np.int32)
        for _ in range(plies):
            self.made = 0
            search = GumbelSearch(self, ids, self.simulations, 4, np.zeros((self.k, self.a), np.float32), 50.0, 0.1)
            search.run(self.net)
            self.t += 1

    def selfplay_stats(self):
        self.calls.append(("selfplay_stats",))
        return np.array([3, 1, 1, 1, 20, self.t], np.int64)

    def selfplay_end(self):
        self.calls.append(("selfplay_end",))


def test_selfplay_session_on_a_stand_in_pool():
    net = Net.random((1, 1, 2), 7, 32, 0, seed=1)
    pool = _StandIn()
    sp = Selfplay(pool, net, dict(policy="gumbel", simulations=8, batch=4, seed=3))
    assert pool.calls[0][0] == "selfplay_begin" and pool.calls[0][1] is net and pool.calls[0][2]["batch"] == 4
    stats = sp.run(3)
    assert stats == Stats(3, 1, 1, 1, 20, 3) and isinstance(stats.games, int)
    assert sp.run(2, wait=False) is None
    assert sp.stats().t == 5
    names = [c[0] for c in pool.calls]
    assert [n for n in names if n.startswith("selfplay")] == ["selfplay_begin", "selfplay_run", "selfplay_stats",
                                                               "selfplay_run", "selfplay_stats"]
    assert ("selfplay_run", 3, True) in pool.calls and ("selfplay_run", 2, False) in pool.calls
    # five plies, each the calls of one `run(net)` round on the stand-in
    per_ply = ["begin"] + ["advance"] * 9 + ["result", "end"]
    assert [n for n in names if not n.startswith("selfplay")] == per_ply * 5
    with pytest.raises(ValueError, match="selfplay_run: plies = 0 must be at least 1"):
        sp.run(0)
    sp.close()
    sp.close()  # (closing twice is fine)
    assert [c[0] for c in pool.calls].count("selfplay_end") == 1
    with pytest.raises(ValueError, match="selfplay: the driver is closed"):
        sp.run(1)
    with pytest.raises(ValueError, match="gumbel_begin: batch = 40"):
        Selfplay(_StandIn(), net, dict(batch=40))
