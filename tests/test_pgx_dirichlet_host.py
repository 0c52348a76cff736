"""PUCT exploration of the PGX self-play driver, CPU side: the contract header envpool_amd/csrc/pgx_dirichlet.hip.h built
for the host by g++ (tests/cpu_harness/pgx_dirichlet_host.cpp) against its numpy restatement
(tests/pgx_dirichlet_util.py), bit for bit; the gamma sampler's distribution; the checks of the Python layer; and the
session on a stand-in pool."""
import ctypes
import math
import os
import statistics
import subprocess

import numpy as np
import pytest

import pgx_dirichlet_util as D
import pgx_selfplay_util as U
from envpool_amd.core import native
from envpool_amd.pgx.net import Net
from envpool_amd.python.envpool import Selfplay
from test_pgx_selfplay_host import _StandIn as _SelfplayStandIn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpu_harness", "pgx_dirichlet_host.cpp")
FLAGS = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"]  # no fast-math, no contraction
F = np.float32
ALPHAS = [0.03, 0.3, 1.0, 3.0, 10.0]
SEED = 0x5EED


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pgx_dirichlet") / "pgx_dirichlet_host.so")
    subprocess.run(FLAGS + ["-shared", "-fPIC", SRC, "-o", out], check=True)
    lib = ctypes.CDLL(out)
    vp, i32, u32, u64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float
    lib.dr_params.argtypes = [f32, vp]
    lib.dr_index.argtypes, lib.dr_index.restype = [i32, i32, i32], i32
    lib.dr_gamma.argtypes = [u64, i32, i32, u32, i32, f32, vp, vp]
    lib.dr_sum.argtypes, lib.dr_sum.restype = [vp, vp, i32], f32
    lib.dr_rows.argtypes, lib.dr_rows.restype = [u64, i32, i32, u32, i32, f32, f32, vp, vp, vp, vp], i32
    lib.dr_weights.argtypes = [i32, i32, vp, f32, vp]
    lib.dr_pick.argtypes, lib.dr_pick.restype = [vp, i32, u32], i32
    lib.dr_move.argtypes = [i32, i32, vp, vp, vp, i32, vp, f32, vp, vp, vp]
    return lib


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def host_gamma(lib, seed, id0, k, t, actions, alpha):
    g, fb = np.zeros((k, actions), F), np.zeros((k, actions), np.int32)
    lib.dr_gamma(seed, id0, k, t, actions, alpha, _ptr(g), _ptr(fb))
    return g, fb


def test_indices_are_apart(lib):
    """The new indices lie above the sample's 0x100 and are pairwise different."""
    seen = set()
    for a in range(127):
        for j in range(D.J):
            for c in (0, 1):
                seen.add(lib.dr_index(a, j, c))
        seen.add(lib.dr_index(a, D.J, 2))
        assert lib.dr_index(a, 3, 1) == int(D.index(a, 3, 1)) == 0x200 + ((a * 16 + 3) * 4 + 1)
    assert len(seen) == 127 * (2 * D.J + 1) and min(seen) == 0x200


@pytest.mark.parametrize("alpha", ALPHAS)
def test_gamma_bit_for_bit(lib, alpha):
    out = np.zeros(3, F)
    lib.dr_params(alpha, _ptr(out))
    assert np.array_equal(bits(out), bits(np.array(D.params(alpha), F)))
    for t in (0, 5):
        g, fb = host_gamma(lib, SEED, 3, 67, t, 65, alpha)
        want, wfb = D.gamma(U.key(SEED, np.arange(3, 70), t), 65, alpha)
        assert np.array_equal(bits(g), bits(want))
        assert np.array_equal(fb != 0, wfb)
        assert (g >= D.FLOOR).all() and np.isfinite(g).all()


def _masks(rng, k, actions):
    """Random masks; row 0 all legal, row 1 one legal action, row 2 none."""
    mask = (rng.random((k, actions)) < 0.6).astype(np.uint8)
    mask[0] = 1
    mask[1] = 0
    mask[1, actions // 2] = 1
    mask[2] = 0
    return mask


@pytest.mark.parametrize("actions", [9, 7, 122, 65])
def test_eta_and_mixed_rows_bit_for_bit(lib, actions):
    rng = np.random.default_rng(actions)
    k, id0 = 11, 5
    mask = _masks(rng, k, actions)
    status = np.zeros(k, np.uint8)
    status[4], status[5] = 1, 2  # rows that are not mixed
    prior = (rng.random((k, actions)).astype(F) * mask).astype(F)
    prior = (prior / np.maximum(prior.sum(axis=1, keepdims=True), F(1e-9))).astype(F)
    for t in (0, 9):
        for alpha, eps in ((0.3, 0.25), (1.0, 0.0), (10.0, 1.0)):
            got_prior, eta = prior.copy(), np.full((k, actions), 7.0, F)
            fallbacks = lib.dr_rows(SEED, id0, k, t, actions, alpha, eps, _ptr(mask), _ptr(status), _ptr(got_prior),
                                    _ptr(eta))
            want_eta, want_fb = D.eta_rows(SEED, np.arange(id0, id0 + k), t, mask, alpha)
            assert np.array_equal(bits(eta), bits(want_eta)) and fallbacks == want_fb
            assert np.array_equal(bits(got_prior), bits(D.mix(prior, want_eta, mask, status, eps)))
            assert eta[1, actions // 2] == 1.0 and not eta[2].any()  # one legal action; none
            assert (eta[mask != 0] > 0).all() and not eta[mask == 0].any()
            assert np.array_equal(bits(got_prior[4:6]), bits(prior[4:6]))  # status 1 and 2: left alone
            assert not got_prior[mask == 0].any()  # illegal entries stay 0
            if eps == 0.0:  # a mix that still draws, and changes nothing
                assert np.array_equal(bits(got_prior), bits(prior)) and eta.any()
    # the sum's order: the harness against the restatement on rows where the order matters
    g = (rng.random((4, actions)) * 3).astype(F)
    full = np.ones(actions, np.uint8)
    for i in range(4):
        assert bits(F(lib.dr_sum(_ptr(g[i]), _ptr(full), actions))) == bits(D.row_sum(g[i:i + 1])[0])


# the largest |float32 row sum - 1| observed over the rows of test_eta_rows_are_positive_and_sum_to_one, in units of
# 2^-24 (half an ulp of 1): 2.384185791015625e-07.  The bound is that plus one ulp of 1
ETA_SUM_OBSERVED_HALF_ULPS = 4


@pytest.fixture(scope="module")
def variates(lib):
    """2^20 variates per alpha: 8192 envs of 128 actions at one ply."""
    return {alpha: host_gamma(lib, SEED, 0, 8192, 1, 128, alpha) for alpha in ALPHAS}


def test_distribution(variates, record_property):
    """Mean and variance of 2^20 Gamma(alpha) variates against alpha and alpha.  The z bound is that of a two-sided
    normal test at a false-alarm rate of 1e-6 over all ten statistics (Bonferroni), from the sample size: the mean's
    standard error is sqrt(alpha / n), the sample variance's sqrt((mu4 - alpha^2) / n) with the fourth central moment
    mu4 = 3 alpha^2 + 6 alpha of Gamma(alpha)."""
    n = 1 << 20
    zmax = statistics.NormalDist().inv_cdf(1.0 - 1e-6 / (2 * len(ALPHAS)) / 2)
    for alpha, (g, fb) in variates.items():
        x = g.astype(np.float64).ravel()
        assert len(x) == n
        a = float(F(alpha))
        z_mean = (x.mean() - a) / math.sqrt(a / n)
        z_var = (x.var(ddof=1) - a) / math.sqrt((2 * a * a + 6 * a) / n)
        print(f"alpha {alpha}: z(mean) {z_mean:+.3f} z(var) {z_var:+.3f} fallbacks {int(fb.sum())}")
        record_property(f"z_{alpha}", (z_mean, z_var))
        assert abs(z_mean) < zmax and abs(z_var) < zmax, (alpha, z_mean, z_var, zmax)
        assert int(fb.sum()) == 0  # none of these draws takes y = d


def test_eta_rows_are_positive_and_sum_to_one(variates):
    """Every legal entry > 0; the float32 sum (in the contract's order) within the largest observed distance from 1
    plus one ulp."""
    worst = 0.0
    for alpha, (g, _) in variates.items():
        for actions in (9, 65, 122):
            gg = np.ascontiguousarray(g[:, :actions])
            S = D.row_sum(gg)
            eta = (gg / S[:, None]).astype(F)
            assert (eta > 0).all()
            worst = max(worst, float(np.abs(D.row_sum(eta).astype(np.float64) - 1.0).max()))
    print(f"largest |sum - 1| = {worst!r} = {worst * 2 ** 24} half ulps")
    assert worst <= ETA_SUM_OBSERVED_HALF_ULPS * 2.0 ** -24 + 2.0 ** -23


def host_move(lib, visits, result_action, elapsed, sample_plies, keys, T):
    visits = np.ascontiguousarray(visits, np.int32)
    k, a = visits.shape
    ra, el = np.ascontiguousarray(result_action, np.int32), np.ascontiguousarray(elapsed, np.int32)
    keys = np.ascontiguousarray(keys, np.uint64)
    action, target, q = np.zeros(k, np.int32), np.zeros((k, a), F), np.zeros((k, a), np.uint32)
    lib.dr_move(k, a, _ptr(visits), _ptr(ra), _ptr(el), sample_plies, _ptr(keys), T, _ptr(action), _ptr(target),
                _ptr(q))
    return action, target, q


HAND_VISITS = np.array([
    [0, 0, 16, 0, 0, 0, 0],      # one action
    [4, 4, 4, 4, 0, 0, 0],       # ties
    [0, 1, 0, 15, 0, 0, 0],      # zeros between
    [1, 2, 3, 4, 5, 6, 7],
    [7, 6, 5, 4, 3, 2, 1],
    [0, 0, 0, 0, 0, 0, 0],       # V == 0
    [3, 0, 0, 0, 0, 0, 13],
    [1, 1, 1, 1, 1, 1, 250],
], np.int32)


@pytest.mark.parametrize("T", [0.25, 0.5, 2.0])
def test_temperature_weights_and_picks(lib, T):
    k, a = HAND_VISITS.shape
    q = np.zeros((k, a), np.uint32)
    lib.dr_weights(k, a, _ptr(HAND_VISITS), T, _ptr(q))
    want = D.weights(HAND_VISITS, T)
    assert np.array_equal(q, want)
    assert (q[HAND_VISITS == 0] == 0).all()
    live = HAND_VISITS.sum(axis=1) > 0
    assert (q.max(axis=1)[live] == 1 << 20).all()  # the most visited action has exactly 2^20
    assert np.array_equal(q[1], [1 << 20] * 4 + [0] * 3)
    # against float64 visits^(1/T): the weights are that within the float32 error of exp_ and log_
    ratio = HAND_VISITS[live] / HAND_VISITS[live].max(axis=1, keepdims=True)
    assert np.abs(q[live] / 2.0 ** 20 - np.where(ratio > 0, ratio ** (1.0 / T), 0.0)).max() < 1e-5
    # r at every prefix boundary: the pick is the lowest action whose inclusive prefix sum exceeds r
    for i in np.flatnonzero(live):
        prefix = np.cumsum(q[i].astype(np.int64))
        for b in np.unique(prefix):
            for r in (b - 1, b):
                if 0 <= r < prefix[-1]:
                    assert lib.dr_pick(_ptr(q[i]), a, int(r)) == int((prefix > r).argmax())
    # the whole move, sampled (elapsed < sample_plies) and greedy, with a root that was over
    keys = U.key(SEED, np.arange(k), 2)
    ra = np.zeros(k, np.int32)
    ra[4] = -1
    for elapsed in (np.zeros(k, np.int32), np.full(k, 4, np.int32), np.arange(k, dtype=np.int32)):
        action, target, _ = host_move(lib, HAND_VISITS, ra, elapsed, 4, keys, T)
        want_action, want_target = D.puct_move_temp(HAND_VISITS, ra, elapsed, 4, keys, T)
        assert np.array_equal(action, want_action) and np.array_equal(bits(target), bits(want_target))
        assert action[0] == 2 and action[5] == 0 and action[4] == 0 and not target[4].any()


def test_temperature_changes_the_draw(lib):
    """The same r lands on other actions under other temperatures: many keys, flat visits against a peak."""
    k = 512
    visits = np.tile(np.array([[8, 1, 1, 1, 1, 1, 1]], np.int32), (k, 1))
    keys = U.key(SEED, np.arange(k), 0)
    zeros = np.zeros(k, np.int32)
    share = {}
    for T in (0.25, 1.0, 2.0):
        action, _, _ = host_move(lib, visits, zeros, zeros, 1, keys, T)
        want, _ = D.puct_move_temp(visits, zeros, zeros, 1, keys, T)
        assert np.array_equal(action, want)
        share[T] = float((action == 0).mean())
    assert share[0.25] > share[1.0] > share[2.0]  # 8^4 : 6, 8 : 6, sqrt(8) : 6
    assert share[0.25] > 0.99 and abs(share[1.0] - 8 / 14) < 0.1 and abs(share[2.0] - 0.32) < 0.1


def test_temperature_one_is_the_plain_move(lib):
    rng = np.random.default_rng(3)
    k, a = 64, 65
    visits = rng.integers(0, 9, (k, a)).astype(np.int32)
    visits[5] = 0
    ra = np.where(rng.random(k) < 0.1, -1, 0).astype(np.int32)
    elapsed = rng.integers(0, 8, k).astype(np.int32)
    keys = U.key(SEED, np.arange(k), 7)
    action, target, q = host_move(lib, visits, ra, elapsed, 4, keys, 1.0)
    want_action, want_target = U.puct_move(visits, ra, elapsed, 4, keys)
    assert np.array_equal(action, want_action) and np.array_equal(bits(target), bits(want_target))
    assert not q.any()


def test_sanitized_program(tmp_path):
    """The harness as a program of its own under the host sanitizers."""
    out = str(tmp_path / "pgx_dirichlet_main")
    subprocess.run(FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DPGX_DIRICHLET_MAIN",
                            SRC, "-o", out], check=True)
    run = subprocess.run([out], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr + run.stdout
    assert "fallbacks 0" in run.stdout


def test_abi_names_and_structs():
    header = open(os.path.join(ROOT, "include", "envpool_amd.h")).read()
    for name in ("epa_selfplay_begin_ex", "epa_selfplay_noise"):
        assert name in native.EXPORTED_SYMBOLS and f"int {name}(" in header
    body = header[header.index("typedef struct epa_selfplay_extra {"):header.index("} epa_selfplay_extra;")]
    fields = [line.split(";")[0].split()[-1] for line in body.splitlines()[1:] if ";" in line]
    assert fields == [f[0] for f in native.SelfplayExtra._fields_]
    assert ctypes.sizeof(native.SelfplayExtra) == 16
    assert ctypes.sizeof(native.SelfplayOptions) == 72  # the options stay as they are


def test_check_selfplay_extra_refusals():
    x = native.check_selfplay_extra()
    assert (x.dirichlet_alpha, x.dirichlet_eps, x.temperature, x.reserved) == (0.0, 0.0, 1.0, 0)  # the plain driver
    x = native.check_selfplay_extra("puct", 0.3, 0.25, 0.5)
    assert (x.dirichlet_alpha, x.dirichlet_eps, x.temperature) == (float(F(0.3)), 0.25, 0.5)
    x = native.check_selfplay_extra("puct", 1, 0.0, 20)  # alpha > 0 with eps == 0: a mix that still draws
    assert (x.dirichlet_alpha, x.dirichlet_eps, x.temperature) == (1.0, 0.0, 20.0)
    assert native.check_selfplay_extra("puct", 100.0, 1.0, 0.05).temperature == float(F(0.05))
    x = native.check_selfplay_extra("gumbel")
    assert (x.dirichlet_alpha, x.dirichlet_eps, x.temperature) == (0.0, 0.0, 1.0)
    bad = [
        (dict(policy="uct"), "selfplay: policy = 'uct' must be 'puct' or 'gumbel'"),
        (dict(dirichlet_alpha=-0.1), "selfplay: dirichlet_alpha = -0.1 must be finite and in 0 .. 100"),
        (dict(dirichlet_alpha=100.5), "selfplay: dirichlet_alpha = 100.5 must be finite"),
        (dict(dirichlet_alpha=float("nan")), "selfplay: dirichlet_alpha = nan must be finite"),
        (dict(dirichlet_alpha=float("inf")), "selfplay: dirichlet_alpha = inf must be finite"),
        (dict(dirichlet_alpha="0.3"), "selfplay: dirichlet_alpha = '0.3' must be a number"),
        (dict(dirichlet_alpha=True), "selfplay: dirichlet_alpha = True must be a number"),
        (dict(dirichlet_eps=-0.01), "selfplay: dirichlet_eps = -0.01 must be in 0 .. 1"),
        (dict(dirichlet_eps=1.5), "selfplay: dirichlet_eps = 1.5 must be in 0 .. 1"),
        (dict(dirichlet_eps=float("nan")), "selfplay: dirichlet_eps = nan must be in 0 .. 1"),
        (dict(temperature=0.04), "selfplay: temperature = 0.04 must be in 0.05 .. 20"),
        (dict(temperature=0.0), "selfplay: temperature = 0.0 must be in 0.05 .. 20"),
        (dict(temperature=20.5), "selfplay: temperature = 20.5 must be in 0.05 .. 20"),
        (dict(temperature=float("nan")), "selfplay: temperature = nan must be in 0.05 .. 20"),
        (dict(temperature=None), "selfplay: temperature = None must be a number"),
        (dict(policy="gumbel", dirichlet_alpha=0.3), r"selfplay: \['dirichlet_alpha'\] are arguments of policy='puct'"),
        (dict(policy="gumbel", dirichlet_eps=0.5), r"selfplay: \['dirichlet_eps'\] are arguments of policy='puct'"),
        (dict(policy="gumbel", temperature=0.5, dirichlet_alpha=1.0),
         r"selfplay: \['dirichlet_alpha', 'temperature'\] are arguments of policy='puct'"),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            native.check_selfplay_extra(**kw)
    # the same refusals through the options of selfplay and arena
    with pytest.raises(ValueError, match="selfplay: temperature = 30 must be in 0.05 .. 20"):
        native.check_selfplay(policy="puct", temperature=30)
    with pytest.raises(ValueError, match="are arguments of policy='puct'"):
        native.check_selfplay(policy="gumbel", dirichlet_alpha=0.3)
    net = Net.random((1, 1, 2), 7, 32, 0, seed=1)
    with pytest.raises(ValueError, match="selfplay: dirichlet_eps = 2 must be in 0 .. 1"):
        native.check_arena(net, net, policy="puct", dirichlet_alpha=0.3, dirichlet_eps=2)
    o = native.check_selfplay(policy="puct", dirichlet_alpha=0.3, temperature=0.5, sample_plies=4)
    assert ctypes.sizeof(o) == 72 and o.sample_plies == 4
    x = native.selfplay_extra_of(dict(policy="puct", dirichlet_alpha=0.3))
    assert (x.dirichlet_alpha, x.dirichlet_eps, x.temperature) == (float(F(0.3)), 0.25, 1.0)
    x = native.selfplay_extra_of(dict(policy="puct"))
    assert (x.dirichlet_alpha, x.dirichlet_eps, x.temperature) == (0.0, 0.0, 1.0)


class _StandIn(_SelfplayStandIn):
    """The self-play tests' stand-in pool with the noise read-out."""

    def selfplay_noise(self):
        self.calls.append(("selfplay_noise",))
        return np.full((self.k, self.a), 0.5, F)


def test_selfplay_session_on_a_stand_in_pool():
    net = Net.random((1, 1, 2), 7, 32, 0, seed=1)
    pool = _StandIn()
    options = dict(policy="puct", simulations=8, seed=3, sample_plies=4, dirichlet_alpha=0.3, dirichlet_eps=0.5,
                   temperature=0.5)
    sp = Selfplay(pool, net, options)
    assert pool.calls[0][0] == "selfplay_begin" and pool.calls[0][2] == options
    assert sp.run(2).t == 2
    noise = sp.noise()
    assert noise.shape == (3, 7) and noise.dtype == F and ("selfplay_noise",) in pool.calls
    sp.close()
    with pytest.raises(ValueError, match="selfplay: the driver is closed"):
        sp.noise()
    with pytest.raises(ValueError, match="selfplay: temperature = 0.01 must be in 0.05 .. 20"):
        Selfplay(_StandIn(), net, dict(policy="puct", temperature=0.01))
    with pytest.raises(ValueError, match=r"selfplay: \['temperature'\] are arguments of policy='puct'"):
        Selfplay(_StandIn(), net, dict(policy="gumbel", temperature=0.5))
