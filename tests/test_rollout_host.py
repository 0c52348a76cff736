"""Rollout collector, CPU side: envpool_amd/csrc/rollout.hip.h built for the host by g++ (a harness that walks the
kernels' blocks and threads as loops) against the contract restated in numpy (rollout_util.Model), bit for bit, on
crafted flag patterns; the store plan at every alignment; the moments against numpy within the summation bound; and
the argument checks of the Python layers, which come before any native call."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rollout_util
from envpool_amd import registration
from envpool_amd.core import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rollout") / "librollouthost.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "cpu_harness", "rollout_host.cpp"), "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.ro_begin.restype = ctypes.c_void_p
    L.ro_buffer.restype = ctypes.c_void_p
    L.ro_step.restype = ctypes.c_int
    L.ro_moments.restype = ctypes.c_int
    for f in (L.ro_end, L.ro_reset, L.ro_next, L.ro_gae, L.ro_counters, L.ro_episodes, L.ro_store_plan, L.ro_copy_span):
        f.restype = None
    return L


# the stored keys: awkward row sizes on purpose (24 B, 147 B, and a 12 B action)
KEYS = [("obs", np.float64, (3,)), ("obs:image", np.uint8, (7, 7, 3)), ("obs:extra", np.float32, (5,))]
ACTION = (np.float32, (3,))


class Harness:
    def __init__(self, L, n, horizon, capacity, id_offset, moments):
        self.L, self.n, self.T = L, n, horizon
        rb = [int(np.prod(s)) * np.dtype(d).itemsize for _, d, s in KEYS] + [int(np.prod(ACTION[1])) * 4]
        dt = [({np.dtype(np.float32): 1, np.dtype(np.float64): 2}.get(np.dtype(d), 0) if moments else 0)
              for _, d, _ in KEYS] + [0]
        self.h = ctypes.c_void_p(L.ro_begin(n, horizon, capacity, id_offset, len(rb), (ctypes.c_int * len(rb))(*rb),
                                            (ctypes.c_int * len(dt))(*dt)))

    def _src(self, arrays):
        self._keep = [np.ascontiguousarray(a) for a in arrays]
        return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in self._keep])

    def reset(self, state):
        ids = np.ascontiguousarray(state["info:env_id"], np.int32)
        self.L.ro_reset(self.h, self.n, ids.ctypes.data_as(ctypes.c_void_p), self._src([state[k] for k, _, _ in KEYS]))

    def step(self, action, state):
        ids = np.ascontiguousarray(state["info:env_id"], np.int32)
        done = np.ascontiguousarray(state["done"], np.uint8)
        trunc = np.ascontiguousarray(state["trunc"], np.uint8)
        rew = np.ascontiguousarray(state["reward"], np.float32)
        rc = self.L.ro_step(self.h, self.n, ids.ctypes.data_as(ctypes.c_void_p), done.ctypes.data_as(ctypes.c_void_p),
                            trunc.ctypes.data_as(ctypes.c_void_p), rew.ctypes.data_as(ctypes.c_void_p),
                            self._src([state[k] for k, _, _ in KEYS] + [action]))
        assert rc == 0

    def array(self, key, dtype, shape):
        p = self.L.ro_buffer(self.h, key)
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return np.frombuffer((ctypes.c_char * n).from_address(p), dtype=dtype).reshape(shape).copy()

    def batch(self, t):
        obs = {k: self.array(i, d, (self.T + 1, self.n, *s))[:t + 1] for i, (k, d, s) in enumerate(KEYS)}
        nk = len(KEYS)
        return (obs, self.array(nk, ACTION[0], (self.T, self.n, *ACTION[1]))[:t],
                self.array(nk + 1, np.float32, (self.T, self.n))[:t], self.array(nk + 2, np.uint8, (self.T, self.n))[:t],
                self.array(nk + 3, np.uint8, (self.T, self.n))[:t], self.array(nk + 4, np.uint8, (self.T, self.n))[:t])

    def counters(self):
        out = (ctypes.c_longlong * 5)()
        self.L.ro_counters(self.h, out)
        return [int(x) for x in out]

    def episodes(self):
        n = self.counters()[0]
        out = (np.empty(n, np.int32), np.empty(n, np.int64), np.empty(n, np.float64), np.empty(n, np.int32))
        self.L.ro_episodes(self.h, *[o.ctypes.data_as(ctypes.c_void_p) for o in out])
        return out

    def gae(self, values, gamma, lam):
        adv, ret = np.empty((self.T, self.n), np.float32), np.empty((self.T, self.n), np.float32)
        v = np.ascontiguousarray(values, np.float32)
        self.L.ro_gae(self.h, v.ctypes.data_as(ctypes.c_void_p), ctypes.c_float(gamma), ctypes.c_float(lam),
                      adv.ctypes.data_as(ctypes.c_void_p), ret.ctypes.data_as(ctypes.c_void_p))
        return adv, ret

    def moments(self, comps):
        out = np.zeros((3, comps))
        assert self.L.ro_moments(self.h, out.ctypes.data_as(ctypes.c_void_p)) == comps
        return out

    def next(self):
        self.L.ro_next(self.h)

    def close(self):
        self.L.ro_end(self.h)


def flags(pattern, n, horizons, rng):
    """(done, trunc) bool [steps, N] for `horizons` horizons of T steps each."""
    steps = sum(horizons)
    done, trunc = np.zeros((steps, n), bool), np.zeros((steps, n), bool)
    if pattern == "ends":            # done at t = 0 and at T - 1 of every horizon
        at = 0
        for t_max in horizons:
            done[at], done[at + t_max - 1] = True, True
            trunc[at + t_max - 1, ::2] = True
            at += t_max
    elif pattern == "twice":         # two dones in a row: the second is the auto-reset row's (length 0)
        done[0::3], done[1::3] = True, True
    elif pattern == "both":          # term and trunc of different envs on the same step
        done[::2] = True
        trunc[::2, ::2] = True
    elif pattern == "all":           # every env done in the same step
        done[steps // 2] = True
        trunc[steps // 2] = rng.random(n) < 0.5
    elif pattern == "random":
        done = rng.random((steps, n)) < 0.3
        trunc = done & (rng.random((steps, n)) < 0.5)
    return done, trunc               # "none": all False


def states(n, steps, done, trunc, id_offset, rng, shuffled):
    """The reset batch and `steps` step batches as a plain pool's recv would return them, and the actions."""
    out = []
    for s in range(steps + 1):
        order = rng.permutation(n) if shuffled else np.arange(n)
        st = {"info:env_id": (order + id_offset).astype(np.int32)}
        for k, d, shape in KEYS:
            x = rng.integers(0, 255, (n, *shape)) if np.dtype(d) == np.uint8 else rng.normal(3.0, 2.0, (n, *shape))
            st[k] = x.astype(d)
        if s > 0:
            st["done"], st["trunc"] = done[s - 1][order], trunc[s - 1][order]
            st["reward"] = rng.normal(0, 1, n).astype(np.float32)
        out.append(st)
    actions = [rng.normal(0, 1, (n, *ACTION[1])).astype(ACTION[0]) for _ in range(steps)]
    return out, actions


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def compare(hs, model, comps):
    t = model.t
    hb, mb = hs.batch(t), model.batch()
    for k in hb[0]:
        assert same(hb[0][k], mb[0][k]), k
    for name, x, y in zip(("action", "reward", "term", "trunc", "mask"), hb[1:], mb[1:]):
        assert same(x, y), name
    if comps:
        assert same(hs.moments(comps), model.mom)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025])
@pytest.mark.parametrize("horizon", [1, 2, 7])
def test_harness_equals_restatement(lib, n, horizon):
    rng = np.random.default_rng(1000 * n + horizon)
    for pi, pattern in enumerate(["ends", "twice", "both", "all", "none", "random"]):
        horizons = [horizon, horizon, horizon]
        done, trunc = flags(pattern, n, horizons, rng)
        shuffled, moments = pi % 2 == 1, n <= 257 and pi in (1, 5)
        capacity = max(1, n // 2) if pattern == "random" else 4 * n * horizon  # (random: the buffer overflows)
        sts, acts = states(n, sum(horizons), done, trunc, 3, rng, shuffled)
        hs = Harness(lib, n, horizon, capacity, 3, moments)
        model = rollout_util.Model(n, horizon, capacity, [k for k, _, _ in KEYS], 3, moments)
        comps = 8 if moments else 0
        hs.reset(sts[0])
        model.reset(sts[0])
        s = 0
        for hi in range(len(horizons)):
            for _ in range(horizon):
                hs.step(acts[s], sts[s + 1])
                model.step(acts[s], sts[s + 1])
                s += 1
            compare(hs, model, comps)
            values = rng.normal(0, 1, (horizon + 1, n)).astype(np.float32)
            for gamma, lam in ((0.99, 0.95), (1.0, 1.0), (0.0, 0.5)):
                ha, ma = hs.gae(values, gamma, lam), model.gae(values, gamma, lam)
                assert same(ha[0], ma[0]) and same(ha[1], ma[1]), (pattern, gamma, lam)
            assert hs.counters()[:4] == [len(model.eps), model.finished, model.dropped, model.steps]
            if hi == 1:  # drained once in the middle: the later horizons append from row 0 again
                for x, y in zip(hs.episodes(), model.episodes()):
                    assert same(x, y), pattern
            hs.next()
            model.next()
        for x, y in zip(hs.episodes(), model.episodes()):
            assert same(x, y), pattern
        if pattern == "random" and n > 1:
            assert model.dropped > 0  # the overflow was hit and counted exactly (the counters above)
        if pattern == "all":
            assert model.finished == n
        hs.close()


def test_mask_and_lengths_on_a_known_pattern(lib):
    """One env, dones at steps 1 and 2: mask is 0 on the step after each done; the second episode has length 0 (its
    only step was the auto-reset row) -- the contract's numbers, not the restatement's."""
    done = np.array([[0], [1], [1], [0], [0]], bool)
    rng = np.random.default_rng(0)
    sts, acts = states(1, 5, done, np.zeros_like(done), 0, rng, False)
    for s in range(1, 6):
        sts[s]["reward"] = np.array([float(s)], np.float32)
    hs = Harness(lib, 1, 5, 8, 0, False)
    hs.reset(sts[0])
    for s in range(5):
        hs.step(acts[s], sts[s + 1])
    _, _, reward, term, trunc, mask = hs.batch(5)
    assert mask[:, 0].tolist() == [1, 1, 0, 0, 1] and term[:, 0].tolist() == [0, 1, 1, 0, 0]
    env, step, ret, length = hs.episodes()
    assert env.tolist() == [0, 0] and step.tolist() == [1, 2] and ret.tolist() == [3.0, 0.0] and length.tolist() == [2, 0]
    hs.close()


def test_gae_known_values(lib):
    """T = 3, one env, gamma = lam = 0.5, reward 1, values 0: plain, terminated, truncated and masked steps by hand."""
    hs = Harness(lib, 1, 3, 0, 0, False)
    rng = np.random.default_rng(0)
    for done, trunc, want in (([0, 0, 0], [0, 0, 0], [1.3125, 1.25, 1.0]),     # a + 0.25 next
                              ([0, 1, 0], [0, 0, 0], [1.25, 1.0, 0.0]),        # term at t = 1; t = 2 is masked
                              ([0, 1, 0], [0, 1, 0], [1.25, 1.0, 0.0])):
        d, tr = np.array(done, bool)[:, None], np.array(trunc, bool)[:, None]
        sts, acts = states(1, 3, d, tr, 0, rng, False)
        hs.reset(sts[0])
        for s in range(3):
            sts[s + 1]["reward"] = np.ones(1, np.float32)
            hs.step(acts[s], sts[s + 1])
        adv, ret = hs.gae(np.zeros((4, 1), np.float32), 0.5, 0.5)
        assert adv[:, 0].tolist() == want and ret[:, 0].tolist() == want
    # a truncated step bootstraps from values[t + 1], a terminated one does not
    v = np.array([[0], [0], [8], [0]], np.float32)
    adv, _ = hs.gae(v, 0.5, 0.5)
    assert adv[1, 0] == 1.0 + 0.5 * 8.0
    hs.close()


def test_store_plan_every_alignment(lib):
    """Head, words and tail of a span for every pair of offsets and every size up to 70; the copy moves exactly the
    span (guard bytes stay) with 1, 64 and 256 threads."""
    src = np.arange(256, dtype=np.uint8)
    base_s = src.ctypes.data
    plan = (ctypes.c_ulonglong * 4)()
    for so in range(17):
        for do in range(17):
            for nbytes in list(range(0, 71)) + [147, 148]:
                lib.ro_store_plan(base_s + so, 4096 + do, nbytes, plan)
                unit, head, words, tail = (int(x) for x in plan)
                if (base_s + so - do) % 16 == 0:
                    assert unit == 16 and head == min(nbytes, -do % 16) and head + 16 * words + tail == nbytes and tail < 16
                elif (base_s + so) % 4 == 0 and do % 4 == 0 and nbytes % 4 == 0:
                    assert (unit, head, 4 * words, tail) == (4, 0, nbytes, 0)
                else:
                    assert (unit, head, words, tail) == (1, nbytes, 0, 0)
                if nbytes % 7 != 0 and nbytes < 147:
                    continue
                for threads in (1, 64, 256):
                    dst = np.full(256, 0xEE, np.uint8)
                    lib.ro_copy_span(ctypes.c_void_p(base_s + so), ctypes.c_void_p(dst.ctypes.data + 32 + do),
                                     ctypes.c_ulonglong(nbytes), threads)
                    want = np.full(256, 0xEE, np.uint8)
                    want[32 + do:32 + do + nbytes] = src[so:so + nbytes]
                    assert np.array_equal(dst, want), (so, do, nbytes, threads)


@pytest.mark.parametrize("n", [1, 255, 257, 1025])
def test_moments_within_the_summation_bound(lib, n):
    """count exact; sum within n u sum|x| and sumsq within 2 n u sum x^2 of numpy's float64 sums over the same rows
    (u = 2^-53): the bound of a summation in any order, where n is the number of rows summed."""
    rng = np.random.default_rng(n)
    horizon = 3
    sts, acts = states(n, horizon, np.zeros((horizon, n), bool), np.zeros((horizon, n), bool), 0, rng, True)
    hs = Harness(lib, n, horizon, 0, 0, True)
    hs.reset(sts[0])
    for s in range(horizon):
        hs.step(acts[s], sts[s + 1])
    mom = hs.moments(8)
    rows = np.concatenate([np.concatenate([st["obs"].astype(np.float64), st["obs:extra"].astype(np.float64)], axis=1)
                           for st in sts])
    total = len(rows)
    assert total == (horizon + 1) * n and np.array_equal(mom[0], np.full(8, float(total)))
    assert np.all(np.abs(mom[1] - rows.sum(axis=0)) <= total * U * np.abs(rows).sum(axis=0))
    assert np.all(np.abs(mom[2] - (rows * rows).sum(axis=0)) <= 2 * total * U * (rows * rows).sum(axis=0))
    # next() does not count slot T twice
    hs.next()
    assert same(hs.moments(8), mom)
    hs.close()


def test_check_rollout_raises_on_each_bad_argument():
    ok = dict(num_envs=8, obs_bytes=24, action_bytes=4)
    assert native.check_rollout(4, 0, False, **ok) == (4, 0, False)
    for horizon in (0, -1, 1.5, True, None, 2 ** 31):
        with pytest.raises(ValueError, match="horizon"):
            native.check_rollout(horizon, 0, False, **ok)
    for episodes in (-1, 0.5, False, None, 2 ** 31):
        with pytest.raises(ValueError, match="episodes"):
            native.check_rollout(4, episodes, False, **ok)
    for moments in (1, None, "yes"):
        with pytest.raises(ValueError, match="moments"):
            native.check_rollout(4, 0, moments, **ok)
    # 65536 envs x 1025 slots x 32 B of observations = 2 GiB + the rest: above the limit; one slot fewer fits
    with pytest.raises(ValueError, match="2 GiB"):
        native.check_rollout(1024, 0, False, 65536, 32, 4)
    assert native.check_rollout(512, 0, False, 65536, 32, 4) == (512, 0, False)
    assert native.rollout_bytes(8, 4, 2, 24, 4) == 5 * 8 * 24 + 4 * 8 * 11 + 48
    with pytest.raises(ValueError, match="2 GiB"):
        native.check_rollout(1, (1 << 31) // 24 + 1, False, 1, 8, 4)
    values = np.zeros((5, 8), np.float32)
    assert native.check_rollout(4, 0, False, 8, values=values, gamma=0.99, lam=1)[4:] == (float(np.float32(0.99)), 1.0)
    for bad in (values.astype(np.float64), values[:4], values[:, :7], values.tolist(), np.zeros((5, 8, 1), np.float32)):
        with pytest.raises(ValueError, match="values"):
            native.check_rollout(4, 0, False, 8, values=bad, gamma=0.99, lam=0.95)
    for gamma, lam in ((-0.1, 0.5), (1.5, 0.5), (0.5, -1), (0.5, 1.01), (float("nan"), 0.5), (None, 0.5), (0.5, "x")):
        with pytest.raises(ValueError, match="gamma|lam"):
            native.check_rollout(4, 0, False, 8, values=values, gamma=gamma, lam=lam)


def test_registry_refuses_pgx_and_atari_ids():
    import envpool_amd  # noqa: F401  (fills the registry)

    ids = registration.list_all_envs()
    for task in ("CartPole-v1", "Pendulum-v1", "Taxi-v3", "HalfCheetah-v4", "MiniGrid-Empty-5x5-v0", "Game2048-v1"):
        assert task in ids and registration.registry.rollout_supported(task)
        registration.registry.check_rollout(task)
    refused = [t for t in ids if not registration.registry.rollout_supported(t)]
    assert any(t.startswith("Pong") for t in refused) and any("tic_tac_toe" in t.lower() or "TicTacToe" in t for t in refused)
    for task in refused:
        assert registration.registry.specs[task][0] in ("envpool_amd.pgx", "envpool_amd.atari")
        with pytest.raises(RuntimeError, match="rollout not implemented for this environment"):
            registration.registry.check_rollout(task)


def test_c_abi_lists_the_rollout_calls():
    names = {"begin", "shape", "reset", "step", "step_device", "view_device", "gae", "gae_device", "episodes",
             "episodes_view_device", "moments", "next", "counters", "end"}
    assert {f"epa_rollout_{n}" for n in names} <= set(native.EXPORTED_SYMBOLS)
    header = open(os.path.join(ROOT, "include", "envpool_amd.h")).read()
    for n in names:
        assert f"int epa_rollout_{n}(" in header


def test_the_licm_fixture_links_every_product_object():
    """tools/build_alt_licm.sh links the product's objects with four of them replaced; its list is kept by hand, and an
    object missing from it (the collector's, once) leaves a library that does not load."""
    import re

    mk = open(os.path.join(ROOT, "envpool_amd", "csrc", "Makefile")).read()
    sh = open(os.path.join(ROOT, "tools", "build_alt_licm.sh")).read()
    product = set(re.search(r"^OBJ = (.*)$", mk, re.M).group(1).split())
    product = {o for o in product if not o.startswith("$(")} | {"build/mujoco_humanoid.o", "build/mujoco_humanoid_standup.o"}
    listed = set(re.search(r'^OBJ="(.*?)"', sh, re.M).group(1).split())
    replaced = {f"build/{tu}.o" for tu in ("mujoco_gym", "mujoco_planar_lg", "mujoco_pusher", "mujoco_ant")}
    assert listed == product - replaced
    for tu in replaced:
        assert tu.replace(".o", "_licm.o") in sh
