"""Rollout actor, CPU side: envpool_amd/csrc/actor.hip.h built for the host by g++ (a harness that walks the kernels'
blocks, threads and lanes as loops) against the contract restated in numpy (actor_util), bit for bit: the feature bytes
of every dtype at the rounding ties, the clamps and the non-finite values, the features kernel's block loop at every
16-byte misalignment, ActorNormal over all 2^23 uniforms, both heads, the sample frequencies, ActorParse's refusals, and
the checks of the Python layers that need no device."""
import ctypes
import os
import statistics
import subprocess

import numpy as np
import pytest

import actor_util as au
import pgx_net_util as nu
from envpool_amd import actor as actor_mod
from envpool_amd.core import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
# ActorNormal against statistics.NormalDist().inv_cdf in float64 over all 2^23 uniforms, as measured with this harness
# (deterministic: no margin); csrc/actor.hip.h and DESIGN.md state the same figures
NORMAL_MAX_ABS = 1.260977683159581e-06
NORMAL_MAX_REL = 3.924487003430764e-07
DTYPES = {np.dtype(np.int32): 0, np.dtype(np.float32): 1, np.dtype(np.float64): 2, np.dtype(np.bool_): 3,
          np.dtype(np.uint8): 4}


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("actor") / "libactorhost.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "cpu_harness", "actor_host.cpp"), "-o", out], check=True)
    L = ctypes.CDLL(out)
    for f in (L.ah_feature, L.ah_features, L.ah_normal, L.ah_normal_all, L.ah_uniform, L.ah_discrete, L.ah_box):
        f.restype = None
    L.ah_parse.restype = L.ah_head.restype = ctypes.c_int
    L.ah_parse.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    L.ah_head.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    L.ah_discrete.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                              ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p,
                              ctypes.c_void_p, ctypes.c_void_p]
    L.ah_box.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_void_p,
                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_longlong,
                         ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.ah_uniform.argtypes = [ctypes.c_ulonglong, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p]
    return L


@pytest.fixture(scope="module")
def normal_all(lib):
    n = 1 << 23
    u, z = np.empty(n, F32), np.empty(n, F32)
    lib.ah_normal_all(vp(u), vp(z))
    return u, z


def harness_features(lib, obs, lo, scale, out=None):
    rows = len(obs[0])
    f = sum(int(np.prod(o.shape[1:], dtype=np.int64)) for o in obs)
    keep = [np.ascontiguousarray(o) for o in obs]
    src = (ctypes.c_void_p * len(obs))(*[o.ctypes.data for o in keep])
    elems = (ctypes.c_int * len(obs))(*[int(np.prod(o.shape[1:], dtype=np.int64)) for o in obs])
    dtype = (ctypes.c_int * len(obs))(*[DTYPES[o.dtype] for o in obs])
    if out is None:
        out = np.zeros((rows, f), np.uint8)
    lo, scale = np.ascontiguousarray(lo, np.float64), np.ascontiguousarray(scale, np.float64)
    lib.ah_features(rows, f, len(obs), src, elems, dtype, vp(lo), vp(scale), vp(out))
    return out


# -- features ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.int32, np.uint8, np.bool_])
def test_feature_bytes_at_ties_clamps_and_non_finite(lib, dtype):
    """lo = 0.5 and scale = 1 put every integer x on a tie x - 0.5 (both parities: half to even); scale = 0.5 puts the
    odd ones on a tie; then both clamps, and for the float dtypes NaN, +-inf and a product that overflows."""
    if np.dtype(dtype).kind == "f":
        x = np.array([0, 1, 2, 3, 4, 5, 0.5, 1.5, 2.5, 126.5, 127.5, 128.5, -0.5, -1e9, 1e9, 200, np.nan, np.inf, -np.inf,
                      np.finfo(dtype).max, -np.finfo(dtype).max], dtype)
    elif dtype is np.bool_:
        x = np.array([0, 1, 1, 0], dtype)
    else:
        x = np.array([0, 1, 2, 3, 4, 5, 126, 127, 128, 129, 255, 200] + ([-1, -2**31, 2**31 - 1] if dtype is np.int32
                                                                          else []), dtype)
    for lo, scale in ((0.5, 1.0), (0.0, 0.5), (0.0, 1.0), (-3.0, 64.0), (0.0, 1e300), (1.0, -1.0)):
        los, scales = np.full(len(x), lo), np.full(len(x), scale)
        want = au.features([x.reshape(1, -1)], los, scales)[0]
        out = np.zeros(len(x), np.uint8)
        lib.ah_feature(vp(np.ascontiguousarray(x, np.float64)), vp(los), vp(scales), len(x), vp(out))
        assert np.array_equal(out, want), (dtype, lo, scale)
        got = harness_features(lib, [x.reshape(1, -1)], los, scales)[0]
        assert np.array_equal(got, want), (dtype, lo, scale)
    if np.dtype(dtype).kind == "f":  # spot values: ties to even, the clamps, non-finite -> 0
        ones, zeros = np.ones(len(x)), np.zeros(len(x))
        got = au.features([x.reshape(1, -1)], zeros, ones)[0]
        assert list(got[6:12]) == [0, 2, 2, 126, 127, 127] and list(got[13:16]) == [0, 127, 127]
        assert list(got[16:19]) == [0, 0, 0]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_features_block_loop_at_every_misalignment(lib, n):
    """Rows of 12 B (float32 [3]), 147 B (uint8 [7, 7, 3]) and 8 * 17 B (float64 [17]): the output row is 167 bytes, so
    blocks start at every offset inside a 16-byte word once the base moves; the base is moved through all 16."""
    rng = np.random.default_rng(n)
    obs = [rng.normal(0, 2, (n, 3)).astype(np.float32), rng.integers(0, 256, (n, 7, 7, 3)).astype(np.uint8),
           rng.normal(0, 2, (n, 17))]
    obs[0][0, 0], obs[2][n - 1, 16] = np.nan, np.inf
    f = 3 + 147 + 17
    lo, scale = rng.uniform(-4, 0, f), rng.uniform(0.3, 20, f)
    want = au.features(obs, lo, scale)
    for shift in range(16):
        raw = np.full(n * f + 64, 0xAB, np.uint8)
        base = (-raw.ctypes.data) % 16 + shift
        out = raw[base:base + n * f].reshape(n, f)
        harness_features(lib, obs, lo, scale, out)
        assert np.array_equal(out, want), shift
        assert (raw[:base] == 0xAB).all() and (raw[base + n * f:] == 0xAB).all()  # nothing outside the span


# -- the inverse normal CDF ------------------------------------------------------------------------------------------------
def test_actor_normal_over_all_uniforms(lib, normal_all):
    u, z = normal_all
    assert np.isfinite(z).all()
    assert (np.diff(z) > 0).all()                      # strictly increasing
    assert np.array_equal(z, -z[::-1])                 # antisymmetric: u - 0.5 and 1 - u are exact
    inv = statistics.NormalDist().inv_cdf
    ref = np.fromiter((inv(float(x)) for x in u.astype(np.float64)), np.float64, len(u))
    err = np.abs(z.astype(np.float64) - ref)
    assert float(err.max()) == NORMAL_MAX_ABS
    assert float((err / np.abs(ref)).max()) == NORMAL_MAX_REL
    sample = np.concatenate([np.arange(0, 1 << 23, 4099), np.arange(64), (1 << 23) - 1 - np.arange(64)])
    assert np.array_equal(au.normal(u[sample]).view(np.uint32), z[sample].view(np.uint32))  # the restatement's bits


def test_uniforms_and_key(lib):
    for seed, env, step in ((0, 0, 0), (7, 1025, 3), (2**63 + 5, 2**31 - 1, 2**40 + 9)):
        out = np.empty(127, F32)
        lib.ah_uniform(seed, env, step, 127, vp(out))
        assert np.array_equal(out, au.uniforms(au.key(seed, [env], step), 127)[0])
        assert (out > 0).all() and (out < 1).all()


# -- the heads -----------------------------------------------------------------------------------------------------------
def head_rows(rng, rows, h):
    """Head integers that give logits of a few units at scale_p = 1/4096, with ties in some rows."""
    p = rng.integers(-12000, 12000, (rows, h + 1)).astype(np.int32)
    p[::5, :h] = p[::5, :1]        # all logits equal: the lowest j wins without noise
    p[1::7, h // 2] = p[1::7, 0]   # a tie between two
    return p


@pytest.mark.parametrize("h", [1, 2, 7, 127])
@pytest.mark.parametrize("deterministic", [False, True])
def test_discrete_head(lib, h, deterministic):
    rng = np.random.default_rng(h)
    rows = 300
    p = head_rows(rng, rows, h)
    ids = (np.arange(rows) + 1000).astype(np.int32)
    sp, sv = F32(1 / 4096), F32(1 / 2048)
    action, logp, value = np.empty(rows, np.int32), np.empty(rows, F32), np.empty(rows, F32)
    lib.ah_discrete(vp(p), rows, h, sp, sv, 11, vp(ids), 5, int(deterministic), vp(action), vp(logp), vp(value))
    wa, wl, wv = au.discrete(p, sp, sv, 11, ids, 5, deterministic)
    assert np.array_equal(action, wa)
    assert np.array_equal(logp.view(np.uint32), wl.view(np.uint32))
    assert np.array_equal(value.view(np.uint32), wv.view(np.uint32))
    if deterministic:
        assert np.array_equal(action, p[:, :h].argmax(axis=1))
    # logp is the log-probability of the action taken: float64 softmax within float32 rounding of the H-term sum
    logit = p[:, :h].astype(np.float64) * float(sp)
    ref = logit[np.arange(rows), action] - np.log(np.exp(logit - logit.max(1, keepdims=True)).sum(1)) - logit.max(1)
    assert np.abs(logp - ref).max() <= (h + 8) * 2.0 ** -23 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("h", [1, 6, 17])
@pytest.mark.parametrize("deterministic", [False, True])
def test_box_head(lib, h, deterministic):
    rng = np.random.default_rng(100 + h)
    rows = 300
    p = head_rows(rng, rows, h)
    ids = (np.arange(rows) + 3).astype(np.int32)
    sp, sv = F32(1 / 4096), F32(1 / 2048)
    sigma = rng.uniform(0.05, 3.0, h).astype(F32)
    low, high = np.full(h, -1.0, F32), np.full(h, 2.0, F32)
    action, logp, value = np.empty((rows, h), F32), np.empty(rows, F32), np.empty(rows, F32)
    lib.ah_box(vp(p), rows, h, sp, sv, vp(sigma), vp(low), vp(high), 2**40 + 1, vp(ids), 9, int(deterministic),
               vp(action), vp(logp), vp(value))
    wa, wl, wv = au.box(p, sp, sv, sigma, low, high, 2**40 + 1, ids, 9, deterministic)
    assert np.array_equal(action.view(np.uint32), wa.view(np.uint32))
    assert np.array_equal(logp.view(np.uint32), wl.view(np.uint32))
    assert np.array_equal(value.view(np.uint32), wv.view(np.uint32))
    assert (action == low).any() and (action == high).any() and ((action > low) & (action < high)).any()
    if deterministic:
        mu = p[:, :h].astype(F32) * sp
        assert np.array_equal(action, np.clip(mu, low, high))


def chi2_sf(x, k):
    """P(chi-square with k degrees of freedom > x), exact: the closed forms of the upper incomplete gamma function for
    integer and half-integer arguments."""
    import math

    y = x / 2.0
    if k % 2 == 0:
        return math.exp(-y) * sum(y ** i / math.factorial(i) for i in range(k // 2))
    return math.erfc(math.sqrt(y)) + math.exp(-y) * sum(y ** (i - 0.5) / math.gamma(i + 0.5)
                                                        for i in range(1, (k - 1) // 2 + 1))


def chi2_quantile(k, alpha):
    """The x with chi2_sf(x, k) = alpha, by bisection on the exact survival function."""
    lo, hi = 0.0, 50.0 + 10.0 * k
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if chi2_sf(mid, k) > alpha else (lo, mid)
    return hi


def test_chi2_quantile_is_exact():
    """k = 1: a squared normal, so the quantile is the square of the normal's two-sided one; k = 2: -2 ln alpha."""
    import math

    assert abs(chi2_quantile(1, 1e-6) - statistics.NormalDist().inv_cdf(1 - 5e-7) ** 2) < 1e-6
    assert abs(chi2_quantile(2, 1e-6) + 2 * math.log(1e-6)) < 1e-9
    assert 23.9 < chi2_quantile(1, 1e-6) < 24.0


@pytest.mark.parametrize("h", [2, 7, 127])
def test_discrete_sample_frequencies(lib, h):
    """2^16 draws of one row (a draw per env id) against softmax(logit): Pearson's chi-square with H - 1 degrees of
    freedom.  The bound is the exact chi-square quantile at a false-alarm rate of 1e-6 (chi2_quantile: 23.93 for
    H = 2, 38.26 for H = 7).  The seed is fixed, so the test is deterministic."""
    rows = 1 << 16
    rng = np.random.default_rng(h)
    logit = rng.normal(0, 1.0, h)
    p1 = np.concatenate([np.rint(logit * 4096), [0]]).astype(np.int32)
    p = np.ascontiguousarray(np.broadcast_to(p1, (rows, h + 1)))
    ids = np.arange(rows, dtype=np.int32)
    action, logp, value = np.empty(rows, np.int32), np.empty(rows, F32), np.empty(rows, F32)
    lib.ah_discrete(vp(p), rows, h, F32(1 / 4096), F32(1), 12345, vp(ids), 0, 0, vp(action), vp(logp), vp(value))
    lg = p1[:h].astype(np.float64) / 4096
    prob = np.exp(lg - lg.max())
    prob /= prob.sum()
    count = np.bincount(action, minlength=h)
    chi2 = float((((count - rows * prob) ** 2) / (rows * prob)).sum())
    bound = chi2_quantile(h - 1, 1e-6)
    assert chi2 <= bound, (chi2, bound)
    assert np.abs(logp.astype(np.float64) - np.log(prob[action])).max() <= (h + 8) * 2.0 ** -23 * np.abs(np.log(prob)).max()


# -- the blob ------------------------------------------------------------------------------------------------------------
def blob_of(f=5, h=3, d=32, blocks=1, kind=0, **kw):
    layers = kw.pop("layers", None) or nu.random_layers(f, h, d, blocks, 0)
    sp, sv = nu.scales(d)
    args = dict(lo=np.zeros(f), scale=np.ones(f), sigma=np.full(h, 0.5, F32))
    args.update(kw)
    return au.make_blob(f, h, d, blocks, kind, layers, sp, sv, **args), layers


def parse(lib, blob):
    blob = np.ascontiguousarray(blob)
    shape = (ctypes.c_int * 5)()
    err = ctypes.create_string_buffer(256)
    ok = lib.ah_parse(vp(blob), blob.nbytes, shape, err, 256)
    return ok, list(shape), err.value.decode()


def test_parse_accepts_and_head_equals_the_restatement(lib):
    for kind in (0, 1):
        blob, layers = blob_of(f=19, h=6, d=64, blocks=2, kind=kind)
        ok, shape, err = parse(lib, blob)
        assert ok == 1 and shape == [19, 6, 64, 2, kind], err
        feat = np.random.default_rng(kind).integers(0, 128, (70, 19)).astype(np.uint8)
        p = np.empty((70, 7), np.int32)
        assert lib.ah_head(vp(blob), blob.nbytes, vp(feat), 70, vp(p)) == 1
        assert np.array_equal(p, au.head(layers, 2, feat))


def test_parse_refusals(lib):
    good, layers = blob_of(kind=1)
    assert parse(lib, good)[0] == 1

    def refused(blob, word):
        ok, _, err = parse(lib, blob)
        assert ok == 0 and word in err, (err, word)

    refused(good[:20], "shorter than a header")
    refused(blob_of(magic=0x4E584750)[0], "magic EPAA")
    refused(blob_of(version=2)[0], "version")
    bad = good.copy()
    bad[24:28] = np.array([2], "<i4").view(np.uint8)
    refused(bad, "kind")
    for field, at, value in (("F", 8, 513), ("F", 8, 0), ("A", 12, 128), ("D", 16, 48), ("L", 20, 9)):
        bad = good.copy()
        bad[at:at + 4] = np.array([value], "<i4").view(np.uint8)
        refused(bad, f"{field} =")
    bad = good.copy()
    bad[28:32] = np.array([np.inf], "<f4").view(np.uint8)
    refused(bad, "scale_p")
    refused(good[:-4], "bytes")
    refused(np.concatenate([good, np.zeros(4, np.uint8)]), "bytes")
    w, b, s = layers[0]
    w = w.copy()
    w[0, 0] = -128
    refused(blob_of(kind=1, layers=[(w, b, s)] + layers[1:])[0], "-128")
    refused(blob_of(kind=1, layers=[(layers[0][0], layers[0][1], 25)] + layers[1:])[0], "shift")
    b2 = layers[1][1].copy()
    b2[0] = 2**30 + 1
    refused(blob_of(kind=1, layers=[layers[0], (layers[1][0], b2, layers[1][2])] + layers[2:])[0], "bias")
    for name in ("lo", "scale"):
        for v in (np.nan, np.inf):
            x = np.ones(5)
            x[3] = v
            refused(blob_of(kind=1, **{name: x})[0], "finite")
    for v in (np.nan, np.inf, 0.0, -1.0):
        sg = np.full(3, 0.5, F32)
        sg[1] = v
        refused(blob_of(kind=1, sigma=sg)[0], "sigma")
    # (a misaligned blob)
    raw = np.zeros(good.nbytes + 8, np.uint8)
    at = (-raw.ctypes.data) % 4 + 1
    raw[at:at + good.nbytes] = good
    ok, _, err = parse(lib, raw[at:at + good.nbytes])
    assert ok == 0 and "aligned" in err


# -- the Python layers, no device ----------------------------------------------------------------------------------------
def test_python_blob_is_the_contracts(lib):
    space = dict(features=11, kind=1, actions=4, low=np.full(4, -1, F32), high=np.full(4, 1, F32),
                 obs_low=np.full(11, -np.inf), obs_high=np.full(11, np.inf))
    a = actor_mod.Actor.random(space, hidden=32, blocks=1, seed=3)
    ok, shape, err = parse(lib, a.blob())
    assert ok == 1 and shape == [11, 4, 32, 1, 1], err
    want = au.make_blob(11, 4, 32, 1, 1, a.net.layers, a.net.scale_p, a.net.scale_v, a.lo, a.scale, a.sigma)
    assert np.array_equal(a.blob(), want)
    obs = [np.random.default_rng(0).normal(0, 4, (40, 11))]
    assert np.array_equal(a.features_of(obs), au.features(obs, a.lo, a.scale))


def test_save_load_and_fit_features(tmp_path):
    space = dict(features=3, kind=0, actions=5, low=np.zeros(0, F32), high=np.zeros(0, F32),
                 obs_low=np.array([-1.0, -np.inf, 0.0]), obs_high=np.array([1.0, np.inf, 3e38]))
    a = actor_mod.Actor.random(space, hidden=32, blocks=0, seed=1)
    assert np.array_equal(a.lo, [-1.0, -8.0, -8.0]) and np.array_equal(a.scale, [63.5, 127 / 16, 127 / 16])
    path = str(tmp_path / "actor.npz")
    a.save(path)
    assert np.array_equal(actor_mod.Actor.load(path).blob(), a.blob())
    x = np.random.default_rng(0).normal([1.0, -2.0, 5.0], [0.5, 2.0, 1.0], (4096, 3))
    a.fit_features(np.full(3, 4096.0), x.sum(0), (x * x).sum(0))
    mean, std = x.mean(0), x.std(0)
    assert np.allclose(a.lo, mean - 4 * std) and np.allclose(a.scale, 127 / (8 * std))
    f = a.features_of([x])
    assert 55 <= f.mean() <= 72 and f.min() >= 0 and f.max() <= 127


def test_refusals_without_a_device():
    import envpool_amd as envpool

    base = dict(kind=0, actions=3, low=np.zeros(0, F32), high=np.zeros(0, F32))
    with pytest.raises(ValueError, match="at most 512"):
        actor_mod.Actor.random(dict(base, features=513, obs_low=np.zeros(513), obs_high=np.ones(513)))
    space = actor_mod.space_of(envpool.make_spec("CartPole-v1"))
    assert (space["features"], space["kind"], space["actions"]) == (4, 0, 2)
    space = actor_mod.space_of(envpool.make_spec("Pendulum-v1"))
    assert (space["features"], space["kind"], space["actions"]) == (3, 1, 1) and space["low"][0] == -2.0
    assert actor_mod.space_of(envpool.make_spec("MiniGrid-Empty-5x5-v0"))["features"] == 1 + 147 + 96
    assert actor_mod.space_of(envpool.make_spec("Taxi-v3"))["features"] == 1
    spec = envpool.make_spec("CartPole-v1")
    for name in ("MultiDiscrete", "Dict"):
        fake = type("S", (), {"state_array_spec": spec.state_array_spec, "action_space": type(name, (), {})()})()
        with pytest.raises(ValueError, match="not supported"):
            actor_mod.space_of(fake)
    a = actor_mod.Actor.random(envpool.make_spec("Pendulum-v1"), hidden=32)
    for sigma in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="sigma"):
            actor_mod.Actor(a.net, 1, a.lo, a.scale, np.full(1, sigma, F32), a.low, a.high)
    with pytest.raises(ValueError, match="finite"):
        actor_mod.Actor(a.net, 1, np.full(3, np.nan), a.scale, a.sigma, a.low, a.high)
    native.check_rollout(32, 0, False, 65536, 982, 4)                    # fits without logp and value ...
    with pytest.raises(ValueError, match="2 GiB"):
        native.check_rollout(32, 0, False, 65536, 982, 4, actor=True)    # ... and is refused with them


def test_symbols_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "envpool_amd.h")).read()
    for name in ("epa_actor_begin", "epa_actor_shape", "epa_actor_end", "epa_actor_eval", "epa_actor_eval_device",
                 "epa_actor_view_device", "epa_actor_batch", "epa_rollout_collect", "epa_rollout_collect_device"):
        assert name in native.EXPORTED_SYMBOLS
        assert f"int {name}(epa_pool* pool" in header
        assert hasattr(native.lib(), name)


# -- the torch twin --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h", [(0, 7), (1, 6)])
def test_torch_twin(lib, kind, h):
    """The twin's integers are the integer forward pass exactly.  Its logp is float64 arithmetic on the float32 logits,
    so what separates it from the contract's float32 logp is the contract's own rounding.  Discrete: H exponentials of
    about 2 ulp each, H - 1 additions and GumbelLog's few ulp on a sum S in [1, H], then one subtraction: at most
    (H + 8) 2^-23 max(1, |logp|).  Box: three operations and a GumbelLog per term and H additions: (5 H + 8) 2^-23
    times the largest partial sum."""
    torch = pytest.importorskip("torch")
    f, rows = 13, 200
    space = dict(features=f, kind=kind, actions=h, low=np.full(h if kind else 0, -1, F32),
                 high=np.full(h if kind else 0, 1, F32), obs_low=np.full(f, -np.inf), obs_high=np.full(f, np.inf))
    a = actor_mod.Actor.random(space, hidden=64, blocks=2, seed=4, sigma=0.7)
    m = a.module()
    rng = np.random.default_rng(5)
    x = rng.normal(0, 5, (rows, f))
    x[0, 0], x[1, 1] = np.nan, np.inf
    feat = au.features([x], a.lo, a.scale)
    assert np.array_equal(m.features(torch.tensor(x)).detach().numpy(), feat.astype(np.float64))
    p = au.head(a.net.layers, 2, feat)
    assert np.array_equal(m.integers(torch.tensor(x)).detach().numpy(), p.astype(np.float64))
    logits, value = m(torch.tensor(x))
    assert np.array_equal(logits.detach().numpy(), p[:, :h].astype(F32) * F32(a.net.scale_p))
    assert np.array_equal(value.detach().numpy(), p[:, h].astype(F32) * F32(a.net.scale_v))
    ids = np.arange(rows, dtype=np.int32)
    sp, sv = F32(a.net.scale_p), F32(a.net.scale_v)
    if kind == 0:
        action, logp, _ = au.discrete(p, sp, sv, 3, ids, 1, False)
        got = m.logp(torch.tensor(x), torch.tensor(action)).detach().numpy()
        assert np.abs(got - logp).max() <= (h + 8) * 2.0 ** -23 * max(1.0, np.abs(logp).max())
    else:
        wide = np.full(h, 1e30, F32)   # no clamp: the action IS the raw one, whose density logp is
        action, logp, _ = au.box(p, sp, sv, a.sigma, -wide, wide, 3, ids, 1, False)
        got = m.logp(torch.tensor(x), torch.tensor(action)).detach().numpy()
        # (the twin recovers z from the rounded raw action: one more rounding of mu + sigma z, relative 2^-24 of |raw|,
        # which enters z^2 / 2 as |z| |raw| 2^-24 / sigma)
        z = np.abs(action - logits.detach().numpy()) / a.sigma
        slack = (z * np.abs(action) / a.sigma).sum(1).max() * 2.0 ** -23
        assert np.abs(got - logp).max() <= (5 * h + 8) * 2.0 ** -23 * np.abs(logp).max() + slack
    ent = m.entropy(torch.tensor(x))
    assert ent.shape == (rows,) and torch.isfinite(ent).all()
    loss = m.logp(torch.tensor(x), torch.tensor(action)).sum() + m.value(torch.tensor(x)).sum()
    loss.backward()
    assert all(w.grad is not None and torch.isfinite(w.grad).all() for w in m.net.weights)
    assert np.array_equal(actor_mod.Actor.from_module(m).blob(), a.blob())
