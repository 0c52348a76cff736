"""A halving level per launch of the PGX Gumbel search on the MI355X: PgxGumbelAdvanceBatch and the batch forms of
begin and result against the host harness of the same header (tests/cpu_harness/pgx_gumbel_batch_host.cpp) fed the
pool's own hidden words and the same evaluator's numbers, for all four games -- leaves after every call, results after
every call; B = 1 against the plain kernels; constant values against a plain session; id order, repeated ids, the
whole pool, a sharded pool; the pool stepped between advances; the device form with a torch model; the refusals
through the wrapper and the raw C ABI; and a pool closed with a batch session open.

The shape: a pool of 70 envs a few plies into their games with one env marked over, 11 ids out of order with one of
them twice (11 blocks of one wave), (S, m, B) = (16, 8, 4) and (32, 16, 16), and (64, 32, 32) once, on Hex."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import envpool_amd as envpool
from envpool_amd.core import native
from envpool_amd.core.device_pool import DevicePool
from pgx_gumbel_batch_util import advances_of_a_round
from pgx_gumbel_util import gumbel_noise, stand_in_logits
from pgx_util import ACTIONS, CODE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMES = ["TicTacToe", "ConnectFour", "Hex", "Othello"]
N, POOL_SEED = 70, 11
PRE = {"TicTacToe": 2, "ConnectFour": 3, "Hex": 3, "Othello": 3}
SHAPE = {"TicTacToe": (3, 3, 2), "ConnectFour": (6, 7, 2), "Hex": (11, 11, 4), "Othello": (8, 8, 2)}
OVER = 33  # the env marked over
IDS = np.array([41, 7, 69, OVER, 0, 64, 12, 63, 7, 50, 22], np.int32)  # out of order, id 7 twice
ALL = np.arange(N, dtype=np.int32)
CASES = [(16, 8, 4), (32, 16, 16)]  # (S, m, B)
F = np.float32


def legal_random(mask, rng):
    mask = np.asarray(mask, bool)
    return (rng.random(mask.shape) * mask + mask).argmax(1).astype(np.int32)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pgx_gumbel_batch") / "libpgxgumbelbatchhost.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "cpu_harness", "pgx_gumbel_batch_host.cpp"), "-o", out], check=True)
    lib = ctypes.CDLL(out)
    lib.pgx_gumbel_batch_begin.restype = ctypes.c_void_p
    lib.pgx_gumbel_batch_result.restype = None
    lib.pgx_gumbel_batch_end.restype = None
    return lib


class Host:
    """The harness's batch session on rows of get_state ([cur_step, done, hidden words])."""

    def __init__(self, lib, fam, st, simulations, considered, batch, gumbel):
        self.lib, self.k, self.n_act = lib, len(st), ACTIONS[fam]
        hid = np.ascontiguousarray(st[:, 2:], np.int32)
        done = np.ascontiguousarray(st[:, 1] != 0, np.uint8)
        gumbel = np.ascontiguousarray(gumbel, F)
        self.obs = np.full((self.k, batch) + SHAPE[fam], 7, np.uint8)
        self.mask = np.full((self.k, batch, self.n_act), 7, np.uint8)
        self.status = np.full((self.k, batch), 7, np.uint8)
        rc = ctypes.c_int(-9)
        self.h = lib.pgx_gumbel_batch_begin(CODE[fam], self.k, _ptr(hid), _ptr(done), simulations, considered, batch,
                                            ctypes.c_float(50.0), ctypes.c_float(0.1), _ptr(gumbel), _ptr(self.obs),
                                            _ptr(self.mask), _ptr(self.status), ctypes.byref(rc))
        assert rc.value == 0 and self.h

    def leaves(self):
        return self.obs.copy(), self.mask.copy(), self.status.copy()

    def advance(self, logits, values):
        logits, values = np.ascontiguousarray(logits, F), np.ascontiguousarray(values, F)
        assert self.lib.pgx_gumbel_batch_advance(ctypes.c_void_p(self.h), _ptr(logits), _ptr(values), _ptr(self.obs),
                                                 _ptr(self.mask), _ptr(self.status)) == 0
        return self.leaves()

    def result(self):
        visits, values = np.full((self.k, self.n_act), -7, np.int32), np.full((self.k, self.n_act), -7, F)
        action, nodes = np.full(self.k, -7, np.int32), np.zeros(self.k, np.int32)
        weights = np.full((self.k, self.n_act), -7, F)
        self.lib.pgx_gumbel_batch_result(ctypes.c_void_p(self.h), _ptr(visits), _ptr(values), _ptr(action),
                                         _ptr(weights), _ptr(nodes))
        return (visits, values, action, weights), nodes

    def close(self):
        self.lib.pgx_gumbel_batch_end(ctypes.c_void_p(self.h))


def same(a, b, what=None):
    """Two tuples of arrays, bit for bit (floats by their bits, bools as bytes)."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape, (what, x.shape, y.shape)
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), np.ascontiguousarray(y, F).view(np.uint32)
        assert np.array_equal(x.view(np.uint8) if x.dtype == np.bool_ else x,
                              y.view(np.uint8) if y.dtype == np.bool_ else y), what


def evaluator(obs, mask):
    """The stand-in evaluator over leaf arrays with or without the slot axis: ([k, B, A], [k, B]) or ([k, A], [k])."""
    lead = mask.shape[:-1]
    logits, values = stand_in_logits(obs.reshape((-1,) + obs.shape[len(lead):]), mask.reshape(-1, mask.shape[-1]))
    return logits.reshape(lead + (-1,)), values.reshape(lead)


def constant(obs, mask):
    logits, values = evaluator(obs, mask)
    return logits, np.zeros_like(values)


def noise_of(fam, ids=IDS, seed=3):
    """Noise per ENV, so that an id listed twice brings the same row twice."""
    return gumbel_noise(seed, N, ACTIONS[fam])[ALL if ids is None else np.asarray(ids)]


class Ctx:
    """One pool per game, a few plies in, env OVER marked over, with its state and snapshot."""

    def __init__(self, fam):
        self.fam = fam
        self.pool = pool = DevicePool(fam, N, seed=POOL_SEED)
        rng = np.random.default_rng(2)
        pool.reset(ALL)
        mask = pool.recv_dict()["info:legal_action_mask"]
        for _ in range(PRE[fam]):
            pool.send(ALL, legal_random(mask, rng))
            mask = pool.recv_dict()["info:legal_action_mask"]
        row = pool.get_state([OVER])
        row[0, 1] = 1.0
        pool.set_state(row, [OVER])
        self.st = pool.get_state()
        self.S = pool.snapshot()
        self.rounds = {}

    def round(self, case, ids=IDS, between=None, evaluate=evaluator):
        """One round through the host forms: the leaves before every call and after the last, the rows fed, the results
        after every call.  `between(t)` runs between two advances."""
        key = (case, tuple(np.asarray(ids).tolist()) if ids is not None else None, evaluate.__name__)
        if between is None and key in self.rounds:
            return self.rounds[key]
        pool, (S, m, B) = self.pool, case
        leaves = pool.gumbel_begin(noise_of(self.fam, ids), ids, S, m, batch=B)
        rec = dict(leaves=[leaves], feed=[], results=[])
        while (leaves[2] != 2).any():
            assert len(rec["feed"]) <= S, "a round is complete after at most S + 1 advances"
            rec["feed"].append(evaluate(leaves[0], leaves[1]))
            leaves = pool.gumbel_advance(*rec["feed"][-1])
            rec["leaves"].append(leaves)
            rec["results"].append(pool.gumbel_result())
            if between is not None:
                between(len(rec["feed"]))
        if between is None:
            assert np.array_equal(pool.get_state(), self.st) and np.array_equal(pool.snapshot(), self.S)
            self.rounds[key] = rec
        return rec


_ctx = {}


def get_ctx(fam):
    if fam not in _ctx:
        _ctx[fam] = Ctx(fam)
    return _ctx[fam]


@pytest.fixture(scope="module", params=GAMES)
def ctx(request):
    return get_ctx(request.param)


def check_against_harness(ctx, harness, case):
    """The kernels against the harness after every call and in the result; the pool byte-identical afterwards (round)."""
    fam, (S, m, B) = ctx.fam, case
    rec = ctx.round(case)
    host = Host(harness, fam, ctx.st[IDS], S, m, B, noise_of(fam))
    want = host.leaves()
    for t, feed in enumerate(rec["feed"]):
        same(rec["leaves"][t], want, (fam, t))
        want = host.advance(*feed)
        res, used = host.result()
        same(rec["results"][t], res, (fam, t))
        assert used.max() <= S + 1
    same(rec["leaves"][-1], want, (fam, "end"))
    obs, mask, status = rec["leaves"][0]
    assert obs.dtype == np.bool_ and mask.dtype == np.bool_ and status.dtype == np.uint8
    assert obs.shape == (len(IDS), B) + SHAPE[fam] and status.shape == (len(IDS), B)
    over = ctx.st[IDS, 1] != 0
    assert over.sum() == 1 and (status[over] == 2).all() and (status[~over, 0] == 0).all() and (status[:, 1:] == 2).all()
    visits, values, action, weights = rec["results"][-1]
    assert visits.dtype == np.int32 and values.dtype == F and action.dtype == np.int32 and weights.dtype == F
    assert (visits[~over].sum(1) == S).all() and (action[over] == -1).all() and not visits[over].any()
    assert not weights[over].any() and np.allclose(weights[~over].sum(1, dtype=np.float64), 1, atol=1e-6)
    legal = mask[:, 0].sum(1)
    want_calls = max(advances_of_a_round(min(m, int(n)), S, B) for n in legal[~over])
    assert len(rec["feed"]) == want_calls and want_calls <= S + 1
    twin = [j for j, e in enumerate(IDS) if e == 7]
    for leaves in rec["leaves"]:
        same([x[twin[0]] for x in leaves], [x[twin[1]] for x in leaves])
    host.close()
    return rec


@pytest.mark.parametrize("case", CASES)
def test_kernels_equal_the_host_harness(ctx, harness, case):
    rec = check_against_harness(ctx, harness, case)
    handed = max((lv[2] != 2).sum(1).max() for lv in rec["leaves"])
    assert handed > 1 and len(rec["feed"]) < case[0] + 1  # fewer calls than the plain session's S + 1


def test_batch_32_on_hex(harness):
    """B = 32 with m = 32, S = 64: picks from both action slots of a lane, a level of 32 in one launch."""
    rec = check_against_harness(get_ctx("Hex"), harness, (64, 32, 32))
    assert max((lv[2] != 2).sum(1).max() for lv in rec["leaves"]) == 32


def test_batch_1_equals_the_plain_kernels(ctx):
    pool, (S, m, _) = ctx.pool, CASES[0]
    rec = ctx.round((S, m, 1))
    assert len(rec["feed"]) == S + 1
    leaves = pool.gumbel_begin(noise_of(ctx.fam), IDS, S, m)
    for t, (logits, values) in enumerate(rec["feed"]):
        same([x[:, 0] for x in rec["leaves"][t]], leaves, (ctx.fam, t))
        leaves = pool.gumbel_advance(logits[:, 0], values[:, 0])
        same(rec["results"][t], pool.gumbel_result(), (ctx.fam, t))
    same([x[:, 0] for x in rec["leaves"][-1]], leaves)
    pool.guided_end()


@pytest.mark.parametrize("fam", ["Hex", "Othello", "ConnectFour"])
def test_constant_values_give_the_plain_sessions_results(fam):
    """From reset, values all 0: sigma is 0 at every node, and every B gives the plain session's results bit for bit."""
    k, S, m = 6, 32, 16
    pool = DevicePool(fam, k, seed=5)
    pool.reset(np.arange(k, dtype=np.int32))
    pool.recv_dict()
    noise = gumbel_noise(9, k, ACTIONS[fam])
    leaves = pool.gumbel_begin(noise, None, S, m)
    for _ in range(S + 1):
        assert not (leaves[2] == 1).any()
        leaves = pool.gumbel_advance(*constant(leaves[0], leaves[1]))
    want = pool.gumbel_result()
    assert (want[0].sum(1) == S).all()
    for B in (4, 16):
        leaves = pool.gumbel_begin(noise, None, S, m, batch=B)
        legal = set(leaves[1][:, 0].sum(1).tolist())
        assert len(legal) == 1  # every env at the start of its game
        calls = 0
        while (leaves[2] != 2).any():
            assert not (leaves[2] == 1).any()  # the condition is checked, not assumed
            leaves = pool.gumbel_advance(*constant(leaves[0], leaves[1]))
            calls += 1
        assert calls == advances_of_a_round(min(m, int(legal.pop())), S, B)
        same(want, pool.gumbel_result(), (fam, B))
    pool.close()


def test_id_order_repeats_and_the_whole_pool(ctx):
    case = CASES[0]
    base = ctx.round(case)
    whole = ctx.round(case, None)
    ids = np.array(sorted(set(IDS.tolist())), np.int32)
    ordered = ctx.round(case, ids)
    assert whole["leaves"][0][0].shape[0] == N
    # every root's search is its own: its rows do not depend on the other rows of the session
    for other, rows in ((whole, IDS), (ordered, np.searchsorted(ids, IDS))):
        calls = min(len(base["feed"]), len(other["feed"]))
        for t in range(calls):
            same(base["leaves"][t], [x[rows] for x in other["leaves"][t]], (ctx.fam, t))
        same(base["results"][-1], [x[rows] for x in other["results"][-1]], ctx.fam)


def test_the_pool_stepped_between_advances(ctx):
    pool, case = ctx.pool, CASES[0]
    base = ctx.round(case)
    rng = np.random.default_rng(4)
    state = {}

    def between(t):
        if t == 1:
            pool.reset(ALL)
            state["mask"] = pool.recv_dict()["info:legal_action_mask"]
        elif t == 3:
            pool.send(ALL, legal_random(state["mask"], rng))
            pool.recv_dict()

    stepped = ctx.round(case, between=between)
    pool.guided_end()
    assert len(stepped["feed"]) == len(base["feed"])
    for t in range(len(base["leaves"])):
        same(base["leaves"][t], stepped["leaves"][t], (ctx.fam, t))
    same(base["results"][-1], stepped["results"][-1])
    pool.restore(ctx.S)
    assert np.array_equal(pool.get_state(), ctx.st)


@pytest.mark.parametrize("fam", ["ConnectFour", "Hex"])
def test_sharded_pool_equals_the_unsharded(fam):
    """device=[0, 0]: two shards, the second with env_id_offset 35, one batch session in each; rows in request order."""
    (S, m, B), results = CASES[0], []
    for device in ([0, 0], 0):
        env = envpool.make(f"{fam}-v1", "gymnasium", num_envs=N, device=device, seed=POOL_SEED)
        rng = np.random.default_rng(2)
        _, info = env.reset()
        for _ in range(PRE[fam]):
            _, _, _, _, info = env.step(legal_random(info["legal_action_mask"], rng))
        gs = env.guided_search(IDS, simulations=S, policy="gumbel", max_considered=m, gumbel=noise_of(fam), batch=B)
        assert gs.leaves[0].shape == (len(IDS), B) + SHAPE[fam] and not gs.done and gs.batch == B
        first, shapes = gs.leaves, []

        def model(obs, mask, status):  # flat rows, as for a plain session
            shapes.append(obs.shape)
            return stand_in_logits(obs, mask)

        out = gs.run(model)
        assert out._fields == ("visits", "values", "action", "weights") and gs.calls < S + 1
        assert set(shapes) == {(len(IDS) * B,) + SHAPE[fam]}
        results.append((out, first, gs.calls))
        env.close()
    same(results[0][0], results[1][0])
    same(results[0][1], results[1][1])
    assert results[0][2] == results[1][2] and results[0][0].visits.sum() == len(IDS) * S


def test_device_form_with_a_model_on_the_device(ctx):
    """gumbel_search_device(batch=) with a small seeded torch model -- until the round is complete (advances=None), and
    with too few advances; the same through the host forms, fed the numbers the model gave."""
    import torch

    from envpool_amd.torch_interop import gumbel_search_device

    pool, fam, n_act, (S, m, B) = ctx.pool, ctx.fam, ACTIONS[ctx.fam], CASES[0]
    k = len(IDS)
    dev = torch.device("cuda", pool.device)
    n_obs = int(np.prod(SHAPE[fam]))
    gen = torch.Generator().manual_seed(3)
    w_p = (torch.randn((n_obs, n_act), generator=gen) * 0.7).to(dev)
    w_v = (torch.randn((n_obs,), generator=gen) * 0.2).to(dev)
    noise = noise_of(fam)
    fed = []

    def evaluate(obs, mask, status):
        assert obs.is_cuda and obs.dtype == torch.bool and mask.dtype == torch.bool and status.dtype == torch.uint8
        assert obs.shape[0] == k * B and status.shape == (k * B,)
        x = obs.reshape(obs.shape[0], -1).float()
        logits, values = x @ w_p, torch.tanh(x @ w_v)
        fed.append((logits.cpu().numpy(), values.cpu().numpy()))
        return logits, values

    def host_forms(feeds):
        pool.gumbel_begin(noise, IDS, S, m, batch=B)
        for logits, values in feeds:
            leaves = pool.gumbel_advance(logits, values)
        out = pool.gumbel_result()
        pool.guided_end()
        return out, leaves

    full = gumbel_search_device(pool, evaluate, IDS, S, m, torch.from_numpy(noise).to(dev), batch=B)
    assert all(t.is_cuda for t in full) and [t.dtype for t in full] == [torch.int32, torch.float32, torch.int32,
                                                                         torch.float32]
    with pytest.raises(ValueError, match="no guided-search session"):  # it closed its session
        pool.guided_end()
    assert len(fed) < S + 1
    want, leaves = host_forms(fed)
    assert (leaves[2] == 2).all()
    same([t.cpu().numpy() for t in full], want, (fam, "full"))
    over = ctx.st[IDS, 1] != 0
    assert (want[0][~over].sum(1) == S).all()
    # an integer that is too small: no host wait, fewer visits, a valid result
    del fed[:]
    few = gumbel_search_device(pool, evaluate, IDS, S, m, torch.from_numpy(noise).to(dev), batch=B, advances=3)
    assert len(fed) == 3
    want, leaves = host_forms(fed)
    same([t.cpu().numpy() for t in few], want, (fam, "few"))
    assert (want[0][~over].sum(1) <= 2 * B).all() and (want[0][~over].sum(1) >= 2).all() and 2 * B < S
    assert (leaves[2][~over] != 2).any()  # roots that are not finished
    for bad in (0, S + 2, 2.5):
        with pytest.raises(ValueError, match="advances"):
            gumbel_search_device(pool, evaluate, IDS, S, m, batch=B, advances=bad)
    with pytest.raises(ValueError, match="advances"):
        gumbel_search_device(pool, evaluate, IDS, S, m, advances=3)
    with pytest.raises(ValueError, match="no guided-search session"):  # none of them opened one
        pool.guided_end()
    assert np.array_equal(pool.get_state(), ctx.st) and np.array_equal(pool.snapshot(), ctx.S)


def _raw_begin_batch(pool, ids, simulations, considered, batch, c_visit=50.0, c_scale=0.1, device=False):
    ids = np.ascontiguousarray(ids, np.int32)
    h, w, c, a = pool.guided_shape()
    n = max(len(ids), 1) * max(min(batch, 32), 1)
    noise = np.zeros((max(len(ids), 1), a), F)
    obs, mask, status = np.zeros((n, h, w, c), np.uint8), np.zeros((n, a), np.uint8), np.zeros(n, np.uint8)
    fn = pool._lib.epa_gumbel_begin_batch_device if device else pool._lib.epa_gumbel_begin_batch
    native.check(fn(pool._h, ids.ctypes.data, len(ids), simulations, considered, batch, ctypes.c_float(c_visit),
                    ctypes.c_float(c_scale), noise.ctypes.data, obs.ctypes.data, mask.ctypes.data, status.ctypes.data))
    return obs, mask, status


def _raw_advance(pool, rows, n_act):
    h, w, c, a = pool.guided_shape()
    n = max(rows, 1)
    logits, values = np.zeros((n, n_act), F), np.zeros(n, F)
    obs, mask, status = np.zeros((n, h, w, c), np.uint8), np.zeros((n, a), np.uint8), np.zeros(n, np.uint8)
    native.check(pool._lib.epa_gumbel_advance(pool._h, logits.ctypes.data, values.ctypes.data, rows, obs.ctypes.data,
                                              mask.ctypes.data, status.ctypes.data))
    return obs, mask, status


def test_refusals_and_the_session_life_cycle():
    cart = DevicePool("CartPole", 4, seed=1)
    buf = np.zeros(4096, np.int32)
    with pytest.raises(RuntimeError, match="gumbel search not implemented"):
        native.check(cart._lib.epa_gumbel_begin_batch(cart._h, buf.ctypes.data, 2, 8, 2, 4, ctypes.c_float(50.0),
                                                      ctypes.c_float(0.1), buf.ctypes.data, buf.ctypes.data,
                                                      buf.ctypes.data, buf.ctypes.data))
    with pytest.raises(RuntimeError, match="gumbel search not implemented"):
        cart.gumbel_begin(np.zeros((4, 2), F), batch=4)
    cart.close()
    ctx = get_ctx("ConnectFour")
    pool, k, n_act, B = ctx.pool, len(IDS), 7, 4
    if getattr(pool, "_guided_k", None) is not None:
        pool.guided_end()
    noise = np.zeros((k, n_act), F)
    # a batch outside 1 .. 32, through the wrapper and the C ABI, both forms; the refusals of the plain forms stay
    for batch in (0, 33, -1):
        with pytest.raises(ValueError, match="gumbel_begin: batch"):
            pool.gumbel_begin(noise, IDS, 8, 4, batch=batch)
        for device in (False, True):
            with pytest.raises(ValueError, match="gumbel_begin: batch"):
                _raw_begin_batch(pool, IDS, 8, 4, batch, device=device)
    for call in (lambda: _raw_begin_batch(pool, IDS, 0, 4, B), lambda: _raw_begin_batch(pool, IDS, 4097, 4, B),
                 lambda: _raw_begin_batch(pool, IDS, 8, 0, B), lambda: _raw_begin_batch(pool, IDS, 8, 4, B, -1.0),
                 lambda: _raw_begin_batch(pool, IDS, 8, 4, B, 50.0, float("inf")),
                 lambda: _raw_begin_batch(pool, IDS[:0], 8, 4, B), lambda: _raw_begin_batch(pool, [70], 8, 4, B),
                 lambda: pool.gumbel_begin(noise, IDS, 0, 4, batch=B),
                 lambda: pool.gumbel_begin(noise[:3], IDS, 8, 4, batch=B)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match="no guided-search session"):  # none of them opened one
        pool.guided_end()
    env = envpool.make("ConnectFour-v1", "gymnasium", num_envs=4, seed=1)
    env.reset()
    for call in (lambda: env.gumbel_search(simulations=8, batch=33), lambda: env.guided_search(simulations=8, batch=2),
                 lambda: env.guided_search(simulations=8, policy="gumbel", batch=0)):
        with pytest.raises(ValueError, match="batch"):
            call()
    for call in (lambda: env.gumbel_search(simulations=8, width=2, batch=2),
                 lambda: env.guided_search(simulations=8, policy="gumbel", width=2)):
        with pytest.raises(ValueError, match="width"):
            call()
    with pytest.raises(ValueError, match="nodes"):
        env.guided_search(simulations=8, policy="gumbel", nodes=20, batch=2)
    gs = env.gumbel_search(simulations=8, batch=1, seed=1)  # batch 1 through the wrapper: the plain session
    assert gs.leaves[2].shape == (4,)
    gs.close()
    env.close()
    # a row count other than k B; reroot; the other policy's calls; none of them changes the session
    leaves = pool.gumbel_begin(noise, IDS, 8, 4, batch=B)
    acts = np.full(k, 3, np.int32)
    calls = 0
    while (leaves[2] != 2).any():
        for rows in (k, k * B - 1, k * B + 1, 0):
            with pytest.raises(ValueError, match="gumbel_advance: logits and values of"):
                _raw_advance(pool, rows, n_act)
        with pytest.raises(ValueError, match="gumbel_advance"):
            pool.gumbel_advance(np.zeros((k, n_act), F), np.zeros(k, F))
        with pytest.raises(ValueError, match="reroot|Gumbel"):
            pool.guided_reroot(acts, 8)
        obs, mask, status = np.zeros((k * B, 6, 7, 2), np.uint8), np.zeros((k * B, 7), np.uint8), np.zeros(k * B, np.uint8)
        with pytest.raises(ValueError, match="reroot not implemented for gumbel sessions"):
            native.check(pool._lib.epa_guided_reroot(pool._h, acts.ctypes.data, k, 8, obs.ctypes.data,
                                                     mask.ctypes.data, status.ctypes.data))
        with pytest.raises(ValueError, match="Gumbel search: use gumbel_"):
            pool.guided_advance(np.zeros((k * B, n_act), F), np.zeros(k * B, F))
        leaves = pool.gumbel_advance(*evaluator(leaves[0], leaves[1]))
        calls += 1
    res = pool.gumbel_result()
    over = ctx.st[IDS, 1] != 0
    assert (res[0][~over].sum(1) == 8).all()
    # later advances on a complete round change nothing, up to call number S; above it they are refused
    zeros = np.zeros((k, B, n_act), F), np.zeros((k, B), F)
    for _ in range(calls, 9):
        leaves = pool.gumbel_advance(*zeros)
        assert (leaves[2] == 2).all() and not leaves[0].any() and not leaves[1].any()
    same(res, pool.gumbel_result())
    with pytest.raises(ValueError, match="call number"):
        pool.gumbel_advance(*zeros)
    # a plain Gumbel session and a PUCT session replace it; the batch rows are then refused
    pool.gumbel_begin(noise, IDS, 4)
    with pytest.raises(ValueError, match="gumbel_advance"):
        pool.gumbel_advance(*zeros)
    pool.guided_begin(IDS, 8, 1.25)
    with pytest.raises(ValueError, match="PUCT guided search: use guided_"):
        pool.gumbel_advance(*zeros)
    pool.guided_end()
    assert np.array_equal(pool.get_state(), ctx.st) and np.array_equal(pool.snapshot(), ctx.S)


def test_trees_above_2_gib_are_refused_and_the_records_count():
    """Hex, S = 63, B = 32: 64 nodes and a record of 32 slots per root; the message names the most roots that fit,
    fewer than a plain session's."""
    node = 80 + 5 * 4 * 124  # (test_pgx_gumbel_host.py: test_node_layout)
    record = 16 + 4 * 124 + 32 * (16 + 4 * 256)  # (test_pgx_gumbel_batch_host.py: the record's layout)
    fits = 2**31 // (64 * node + record)
    assert fits + 8 < 2**31 // (64 * node)
    pool = DevicePool("Hex", fits + 8, seed=1)
    ids = np.arange(fits + 8, dtype=np.int32)
    pool.reset(ids)
    pool.recv_dict()
    st = pool.get_state()
    noise = np.zeros((fits + 1, 122), F)
    with pytest.raises(ValueError, match=f"at most {fits} roots"):
        pool.gumbel_begin(noise, ids[:fits + 1], 63, 16, batch=32)
    import torch

    d = torch.zeros(16, dtype=torch.float32, device=torch.device("cuda", pool.device)).data_ptr()  # (never used)
    with pytest.raises(ValueError, match=f"at most {fits} roots"):
        pool.gumbel_begin_device(d, d, d, d, ids[:fits + 1], 63, 16, batch=32)
    with pytest.raises(ValueError, match="no guided-search session"):
        pool.guided_end()
    assert np.array_equal(pool.get_state(), st)
    pool.close()


def test_closing_a_pool_with_a_batch_session_open():
    pool = DevicePool("Othello", 8, seed=3)
    pool.reset(np.arange(8, dtype=np.int32))
    pool.recv_dict()
    noise = gumbel_noise(2, 8, 65)
    leaves = pool.gumbel_begin(noise, None, 16, 8, batch=8)
    leaves = pool.gumbel_advance(*evaluator(leaves[0], leaves[1]))
    assert (leaves[2] == 0).sum() > 8
    pool.close()
    again = DevicePool("Othello", 8, seed=3)  # and a new pool works
    again.reset(np.arange(8, dtype=np.int32))
    again.recv_dict()
    first = again.gumbel_begin(noise, None, 16, 8, batch=8)
    same(again.gumbel_advance(*evaluator(first[0], first[1])), leaves)
    again.close()


def teardown_module(module):
    for c in _ctx.values():
        c.pool.close()
    _ctx.clear()
