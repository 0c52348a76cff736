"""Several leaves per launch of the PGX guided search on the MI355X: PgxGuidedAdvanceWide and the wide variants of
begin, result and reroot against the host harness of the same header
(tests/cpu_harness/pgx_guided_wide_host.cpp) fed the pool's own hidden words and the same evaluator's numbers, for all
four games -- leaves after every call, results after every call; width 1 against the plain kernels; id order, repeated
ids, the whole pool, a sharded pool; the pool stepped between advances; the device form with a torch model; reroot
through both forms; the refusals through the wrapper and the raw C ABI; and the session's life cycle.

The shape: a pool of 70 envs a few plies into their games with one env marked over, 11 ids out of order with one of
them twice (11 blocks of one wave), S = 24 simulations (Hex: S = 12), width 4 -- width 16 on TicTacToe and Hex and
width 32 once, on TicTacToe (the kernel's three path buckets) -- and 3 roots at the capacities of the reroot kernel's two
larger tables."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import envpool_amd as envpool
from envpool_amd.core import native
from envpool_amd.core.device_pool import DevicePool
from pgx_guided_util import stand_in
from pgx_util import ACTIONS, CODE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMES = ["TicTacToe", "ConnectFour", "Hex", "Othello"]
N, POOL_SEED, C_PUCT, W = 70, 11, 1.25, 4
SIMS = {"TicTacToe": 24, "ConnectFour": 24, "Hex": 12, "Othello": 24}
PRE = {"TicTacToe": 2, "ConnectFour": 3, "Hex": 3, "Othello": 3}
SHAPE = {"TicTacToe": (3, 3, 2), "ConnectFour": (6, 7, 2), "Hex": (11, 11, 4), "Othello": (8, 8, 2)}
OVER = 33  # the env marked over
IDS = np.array([41, 7, 69, OVER, 0, 64, 12, 63, 7, 50, 22], np.int32)  # out of order, id 7 twice
ALL = np.arange(N, dtype=np.int32)
F = np.float32


def legal_random(mask, rng):
    mask = np.asarray(mask, bool)
    return (rng.random(mask.shape) * mask + mask).argmax(1).astype(np.int32)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pgx_wide") / "libpgxwidehost.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "cpu_harness", "pgx_guided_wide_host.cpp"), "-o", out], check=True)
    lib = ctypes.CDLL(out)
    lib.pgx_wide_begin.restype = ctypes.c_void_p
    lib.pgx_wide_result.restype = None
    lib.pgx_wide_end.restype = None
    return lib


class Host:
    """The harness's wide session on rows of get_state ([cur_step, done, hidden words])."""

    def __init__(self, lib, fam, st, simulations, nodes, width, c_puct):
        self.lib, self.k, self.n_act = lib, len(st), ACTIONS[fam]
        hid = np.ascontiguousarray(st[:, 2:], np.int32)
        done = np.ascontiguousarray(st[:, 1] != 0, np.uint8)
        self.obs = np.full((self.k, width) + SHAPE[fam], 7, np.uint8)
        self.mask = np.full((self.k, width, self.n_act), 7, np.uint8)
        self.status = np.full((self.k, width), 7, np.uint8)
        rc = ctypes.c_int(-9)
        self.h = lib.pgx_wide_begin(CODE[fam], self.k, _ptr(hid), _ptr(done), simulations, nodes or simulations + 1,
                                    width, ctypes.c_float(c_puct), _ptr(self.obs), _ptr(self.mask), _ptr(self.status),
                                    ctypes.byref(rc))
        assert rc.value == 0 and self.h

    def leaves(self):
        return self.obs.copy(), self.mask.copy(), self.status.copy()

    def advance(self, priors, values):
        priors, values = np.ascontiguousarray(priors, F), np.ascontiguousarray(values, F)
        assert self.lib.pgx_wide_advance(ctypes.c_void_p(self.h), _ptr(priors), _ptr(values), _ptr(self.obs),
                                         _ptr(self.mask), _ptr(self.status)) == 0
        return self.leaves()

    def reroot(self, actions, simulations):
        actions = np.ascontiguousarray(actions, np.int32)
        assert self.lib.pgx_wide_reroot(ctypes.c_void_p(self.h), _ptr(actions), simulations, _ptr(self.obs),
                                        _ptr(self.mask), _ptr(self.status)) == 0
        return self.leaves()

    def result(self):
        visits, values = np.full((self.k, self.n_act), -7, np.int32), np.full((self.k, self.n_act), -7, F)
        action, nodes, done = np.full(self.k, -7, np.int32), np.zeros(self.k, np.int32), np.zeros(self.k, np.int32)
        self.lib.pgx_wide_result(ctypes.c_void_p(self.h), _ptr(visits), _ptr(values), _ptr(action), _ptr(nodes),
                                 _ptr(done))
        return (visits, values, action), nodes, done

    def close(self):
        self.lib.pgx_wide_end(ctypes.c_void_p(self.h))


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
    """The stand-in evaluator over leaf arrays with the slot axis: ([k, W, A], [k, W])."""
    lead = mask.shape[:-1]
    priors, values = stand_in(obs.reshape((-1,) + obs.shape[len(lead):]), mask.reshape(-1, mask.shape[-1]))
    return priors.reshape(lead + (-1,)), values.reshape(lead)


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

    def round(self, ids=IDS, width=W, nodes=0, between=None):
        """One round through the host forms: the leaves before every call and after the last, the rows fed, the results
        after every call.  `between(t)` runs between two advances."""
        key = (tuple(np.asarray(ids).tolist()) if ids is not None else None, width, nodes)
        if between is None and key in self.rounds:
            return self.rounds[key]
        pool, S = self.pool, SIMS[self.fam]
        leaves = pool.guided_begin(ids, S, C_PUCT, nodes, width)
        rec = dict(leaves=[leaves], feed=[], results=[])
        while (leaves[2] != 2).any():
            assert len(rec["feed"]) <= S, "a round is complete after at most S + 1 advances"
            rec["feed"].append(evaluator(leaves[0], leaves[1]))
            leaves = pool.guided_advance(*rec["feed"][-1])
            rec["leaves"].append(leaves)
            rec["results"].append(pool.guided_result())
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


def check_against_harness(ctx, harness, width, nodes=0):
    fam, S = ctx.fam, SIMS[ctx.fam]
    rec = ctx.round(IDS, width, nodes)
    host = Host(harness, fam, ctx.st[IDS], S, nodes, width, C_PUCT)
    want = host.leaves()
    for t, feed in enumerate(rec["feed"]):
        same(rec["leaves"][t], want, (fam, t))
        want = host.advance(*feed)
        res, used, done = host.result()
        same(rec["results"][t], res, (fam, t))
        assert (res[0].sum(1) == done).all() and used.max() <= (nodes or S + 1)
    same(rec["leaves"][-1], want, (fam, "end"))
    obs, mask, status = rec["leaves"][0]
    assert obs.dtype == np.bool_ and mask.dtype == np.bool_ and status.dtype == np.uint8
    assert obs.shape == (len(IDS), width) + SHAPE[fam] and status.shape == (len(IDS), width)
    over = ctx.st[IDS, 1] != 0
    assert over.sum() == 1 and (status[over] == 2).all() and (status[~over, 0] == 0).all() and (status[:, 1:] == 2).all()
    (visits, values, action), _, done = host.result()
    assert (visits[~over].sum(1) == S).all() and (done[~over] == S).all() and (action[over] == -1).all()
    assert not visits[over].any() and len(rec["feed"]) <= S + 1
    twin = [j for j, e in enumerate(IDS) if e == 7]
    for leaves in rec["leaves"]:
        same([x[twin[0]] for x in leaves], [x[twin[1]] for x in leaves])
    host.close()
    return rec


def test_kernels_equal_the_host_harness(ctx, harness):
    rec = check_against_harness(ctx, harness, W)
    handed = [(lv[2] != 2).sum(1).max() for lv in rec["leaves"]]
    assert max(handed) == W and len(rec["feed"]) < SIMS[ctx.fam] + 1  # fewer calls than the plain session's S + 1


def test_width_32_on_tictactoe(harness):
    rec = check_against_harness(get_ctx("TicTacToe"), harness, 32)
    assert max((lv[2] != 2).sum(1).max() for lv in rec["leaves"]) > W


@pytest.mark.parametrize("fam", ["TicTacToe", "Hex"])
def test_width_16(harness, fam):
    """The middle path bucket of PgxGuidedAdvanceWide (5 .. 16 slots), with one and with two action slots per lane."""
    check_against_harness(get_ctx(fam), harness, 16)


@pytest.mark.parametrize("fam,nodes", [("ConnectFour", 513), ("ConnectFour", 2049), ("ConnectFour", 8192),
                                       ("Hex", 513), ("Hex", 2049)])
def test_the_larger_reroot_tables_equal_the_harness(harness, fam, nodes):
    """The wide PgxGuidedReroot with its 2048- and 8192-entry tables (capacities above 512 and above 2048): 3 roots of
    width 4, a round of 8 simulations, a reroot by the chosen moves and a second round -- leaves after every call,
    results after both rounds and after the reroot, bit for bit."""
    ctx = get_ctx(fam)
    pool, S, ids = ctx.pool, 8, IDS[:3]
    assert OVER not in ids
    host = Host(harness, fam, ctx.st[ids], S, nodes, W, C_PUCT)
    leaves = pool.guided_begin(ids, S, C_PUCT, nodes, W)
    same(leaves, host.leaves(), (fam, "begin"))
    for move in range(2):
        calls = 0
        while (leaves[2] != 2).any():
            feed = evaluator(leaves[0], leaves[1])
            leaves = pool.guided_advance(*feed)
            same(leaves, host.advance(*feed), (fam, move, calls))
            calls += 1
            assert calls <= S + 1
        res = pool.guided_result()
        same(res, host.result()[0], (fam, move))
        if move == 0:
            sent = np.where(res[2] < 0, 0, res[2]).astype(np.int32)
            assert (res[0][np.arange(3), sent] >= 1).all()  # the most visited move has a child: the table path
            leaves = pool.guided_reroot(sent, S)
            same(leaves, host.reroot(sent, S), (fam, "reroot"))
            same(pool.guided_result(), host.result()[0], (fam, "kept"))
    pool.guided_end()
    host.close()
    assert np.array_equal(pool.get_state(), ctx.st) and np.array_equal(pool.snapshot(), ctx.S)


def test_a_roomy_session_and_reroot_equal_the_harness(ctx, harness):
    """nodes = 2 S + 1, the round, a host-form reroot by the chosen moves, and the next round."""
    fam, S, pool = ctx.fam, SIMS[ctx.fam], ctx.pool
    nodes = 2 * S + 1
    rec = check_against_harness(ctx, harness, W, nodes)
    host = Host(harness, fam, ctx.st[IDS], S, nodes, W, C_PUCT)
    leaves = pool.guided_begin(IDS, S, C_PUCT, nodes, W)
    for feed in rec["feed"]:
        leaves = pool.guided_advance(*feed)
        host.advance(*feed)
    action = pool.guided_result()[2]
    sent = np.where(action < 0, 0, action).astype(np.int32)
    leaves = pool.guided_reroot(sent, S - 2)
    same(leaves, host.reroot(sent, S - 2), (fam, "reroot"))
    kept = pool.guided_result()
    same(kept, host.result()[0], (fam, "kept"))
    assert (leaves[2][:, 1:] == 2).all() and set(np.unique(leaves[2][:, 0])) <= {0, 2}
    calls = 0
    while (leaves[2] != 2).any():
        feed = evaluator(leaves[0], leaves[1])
        leaves = pool.guided_advance(*feed)
        same(leaves, host.advance(*feed), (fam, "round 2", calls))
        calls += 1
        assert calls <= S - 1
    res, used, done = host.result()
    same(pool.guided_result(), res, (fam, "round 2"))
    still = kept[2] >= 0
    assert (done[still] == S - 2).all() and (used <= nodes).all() and not done[~still].any()
    assert (res[0][still].sum(1) == kept[0][still].sum(1) + S - 2).all()  # the kept visits add to the round's S2
    pool.guided_end()
    host.close()
    assert np.array_equal(pool.get_state(), ctx.st) and np.array_equal(pool.snapshot(), ctx.S)


def test_width_1_wide_equals_the_plain_kernels(ctx):
    pool, S = ctx.pool, SIMS[ctx.fam]
    rec = ctx.round(IDS, 1)
    assert len(rec["feed"]) == S + 1
    leaves = pool.guided_begin(IDS, S, C_PUCT)
    for t, (priors, values) in enumerate(rec["feed"]):
        same([x[:, 0] for x in rec["leaves"][t]], leaves, (ctx.fam, t))
        leaves = pool.guided_advance(priors[:, 0], values[:, 0])
        same(rec["results"][t], pool.guided_result(), (ctx.fam, t))
    same([x[:, 0] for x in rec["leaves"][-1]], leaves)
    pool.guided_end()


def test_id_order_repeats_and_the_whole_pool(ctx):
    base = ctx.round(IDS, W)
    whole = ctx.round(None, W)
    ids = np.array(sorted(set(IDS.tolist())), np.int32)
    ordered = ctx.round(ids, W)
    assert whole["leaves"][0][0].shape[0] == N
    # every root's search is its own: its rows do not depend on the other rows of the session
    for other, rows in ((whole, IDS), (ordered, np.searchsorted(ids, IDS))):
        calls = min(len(base["feed"]), len(other["feed"]))
        for t in range(calls):
            same(base["leaves"][t], [x[rows] for x in other["leaves"][t]], (ctx.fam, t))
        same(base["results"][-1], [x[rows] for x in other["results"][-1]], ctx.fam)


def test_the_pool_stepped_between_advances(ctx):
    pool = ctx.pool
    base = ctx.round(IDS, W)
    rng = np.random.default_rng(4)

    state = {}

    def between(t):
        if t == 1:
            pool.reset(ALL)
            state["mask"] = pool.recv_dict()["info:legal_action_mask"]
        elif t == 3:
            pool.send(ALL, legal_random(state["mask"], rng))
            pool.recv_dict()

    stepped = ctx.round(IDS, W, between=between)
    pool.guided_end()
    assert len(stepped["feed"]) == len(base["feed"])
    for t in range(len(base["leaves"])):
        same(base["leaves"][t], stepped["leaves"][t], (ctx.fam, t))
    same(base["results"][-1], stepped["results"][-1])
    pool.restore(ctx.S)
    assert np.array_equal(pool.get_state(), ctx.st)


@pytest.mark.parametrize("fam", ["ConnectFour", "Hex"])
def test_sharded_pool_equals_the_unsharded(fam):
    """device=[0, 0]: two shards, the second with env_id_offset 35, one wide session in each; rows in request order."""
    S, results = SIMS[fam], []
    for device in ([0, 0], 0):
        env = envpool.make(f"{fam}-v1", "gymnasium", num_envs=N, device=device, seed=POOL_SEED)
        rng = np.random.default_rng(2)
        _, info = env.reset()
        for _ in range(PRE[fam]):
            _, _, _, _, info = env.step(legal_random(info["legal_action_mask"], rng))
        gs = env.guided_search(IDS, simulations=S, c_puct=C_PUCT, nodes=2 * S + 1, width=W)
        assert gs.leaves[0].shape == (len(IDS), W) + SHAPE[fam] and not gs.done
        shapes, rec = [], []

        def model(obs, mask, status):  # flat rows, as for a plain session
            shapes.append(obs.shape)
            return stand_in(obs, mask)

        for move in range(2):
            out = gs.run(model, close=False)
            assert gs.done and gs.calls < S + 1
            rec.append((out, gs.reroot(out.action)))
            assert gs.calls == 0 and not gs.done
        gs.close()
        assert set(shapes) == {(len(IDS) * W,) + SHAPE[fam]}
        results.append(rec)
        env.close()
    for (a, la), (b, lb) in zip(*results):
        same(a, b)
        same(la, lb)
    assert results[0][1][0].visits.sum() > results[0][0][0].visits.sum() == len(IDS) * S  # the kept visits count


def test_device_form_with_a_model_on_the_device(ctx):
    """guided_search_device(width=) with a small seeded torch model -- until the round is complete (advances=None), and
    with too few advances -- then guided_reroot_device; the same through the host forms, fed the numbers the model gave."""
    import torch

    from envpool_amd.torch_interop import guided_reroot_device, guided_search_device

    pool, fam, n_act, S = ctx.pool, ctx.fam, ACTIONS[ctx.fam], SIMS[ctx.fam]
    nodes, k = 2 * S + 1, len(IDS)
    dev = torch.device("cuda", pool.device)
    n_obs = int(np.prod(SHAPE[fam]))
    gen = torch.Generator().manual_seed(3)
    w_p = (torch.randn((n_obs, n_act), generator=gen) * 0.3).to(dev)
    w_v = (torch.randn((n_obs,), generator=gen) * 0.2).to(dev)
    fed = []

    def evaluate(obs, mask, status):
        assert obs.is_cuda and obs.dtype == torch.bool and mask.dtype == torch.bool and status.dtype == torch.uint8
        assert obs.shape[0] == k * W and status.shape == (k * W,)
        x = obs.reshape(obs.shape[0], -1).float()
        priors, values = torch.softmax(x @ w_p, dim=1) * mask.float(), torch.tanh(x @ w_v)
        fed.append((priors.cpu().numpy(), values.cpu().numpy()))
        return priors, values

    def host_forms(feeds, reroot=None):
        pool.guided_begin(IDS, S, C_PUCT, nodes, W)
        out = []
        for i, (priors, values) in enumerate(feeds):
            if reroot is not None and i == reroot[0]:
                out.append(pool.guided_result())
                pool.guided_reroot(reroot[1], S)
            leaves = pool.guided_advance(priors, values)
        out.append(pool.guided_result())
        pool.guided_end()
        return out, leaves

    # until the round is complete, then a reroot by the chosen moves and a second round
    first = guided_search_device(pool, evaluate, IDS, S, C_PUCT, nodes=nodes, keep_open=True, width=W)
    n1 = len(fed)
    assert n1 < S + 1 and all(t.is_cuda for t in first)
    actions = torch.where(first[2] < 0, torch.zeros_like(first[2]), first[2])
    second = guided_reroot_device(pool, evaluate, actions, S)
    pool.guided_end()
    want, leaves = host_forms(fed, (n1, actions.cpu().numpy()))
    assert (leaves[2] == 2).all()
    same([t.cpu().numpy() for t in first], want[0], (fam, "first"))
    same([t.cpu().numpy() for t in second], want[1], (fam, "second"))
    over = ctx.st[IDS, 1] != 0
    assert (want[0][0][~over].sum(1) == S).all()
    # an integer that is too small: no host wait, fewer visits, a valid result
    del fed[:]
    few = guided_search_device(pool, evaluate, IDS, S, C_PUCT, nodes=nodes, width=W, advances=3)
    assert len(fed) == 3
    want, leaves = host_forms(fed)
    visits, values, action = [t.cpu().numpy() for t in few]
    same((visits, values, action), want[0], (fam, "few"))
    assert (visits[~over].sum(1) <= 2 * W).all() and (visits[~over].sum(1) >= 2).all() and 2 * W < S
    assert (leaves[2][~over] != 2).any()  # roots that are not finished
    legal = ctx.round(IDS, W)["leaves"][0][1][:, 0]
    assert legal[~over][np.arange((~over).sum()), action[~over]].all() and (action[over] == -1).all()
    for bad in (0, S + 2, 2.5):
        with pytest.raises(ValueError, match="advances"):
            guided_search_device(pool, evaluate, IDS, S, C_PUCT, width=W, advances=bad)
    with pytest.raises(ValueError, match="advances"):
        guided_search_device(pool, evaluate, IDS, S, C_PUCT, advances=3)
    assert np.array_equal(pool.get_state(), ctx.st) and np.array_equal(pool.snapshot(), ctx.S)


def _raw_begin_wide(pool, ids, simulations, nodes, width, c_puct, device=False):
    ids = np.ascontiguousarray(ids, np.int32)
    h, w, c, a = pool.guided_shape()
    n = max(len(ids), 1) * max(min(width, 32), 1)
    obs, mask, status = np.zeros((n, h, w, c), np.uint8), np.zeros((n, a), np.uint8), np.zeros(n, np.uint8)
    fn = pool._lib.epa_guided_begin_wide_device if device else pool._lib.epa_guided_begin_wide
    native.check(fn(pool._h, ids.ctypes.data, len(ids), simulations, nodes, width, ctypes.c_float(c_puct),
                    obs.ctypes.data, mask.ctypes.data, status.ctypes.data))
    return obs, mask, status


def _raw_advance(pool, rows, n_act):
    h, w, c, a = pool.guided_shape()
    n = max(rows, 1)
    priors, values = np.zeros((n, n_act), F), np.zeros(n, F)
    obs, mask, status = np.zeros((n, h, w, c), np.uint8), np.zeros((n, a), np.uint8), np.zeros(n, np.uint8)
    native.check(pool._lib.epa_guided_advance(pool._h, priors.ctypes.data, values.ctypes.data, rows, obs.ctypes.data,
                                              mask.ctypes.data, status.ctypes.data))
    return obs, mask, status


def _raw_reroot(pool, actions, k, simulations, width):
    actions = np.ascontiguousarray(actions, np.int32)
    h, w, c, a = pool.guided_shape()
    n = max(k, 1) * width
    obs, mask, status = np.zeros((n, h, w, c), np.uint8), np.zeros((n, a), np.uint8), np.zeros(n, np.uint8)
    native.check(pool._lib.epa_guided_reroot(pool._h, actions.ctypes.data, k, simulations, obs.ctypes.data,
                                             mask.ctypes.data, status.ctypes.data))
    return obs, mask, status


def test_refusals_and_the_session_life_cycle():
    cart = DevicePool("CartPole", 4, seed=1)
    buf = np.zeros(4096, np.int32)
    with pytest.raises(RuntimeError, match="guided search not implemented"):
        native.check(cart._lib.epa_guided_begin_wide(cart._h, buf.ctypes.data, 2, 8, 0, 4, ctypes.c_float(1.0),
                                                     buf.ctypes.data, buf.ctypes.data, buf.ctypes.data))
    with pytest.raises(RuntimeError, match="guided search not implemented"):
        cart.guided_begin(None, 8, C_PUCT, 0, 4)
    cart.close()
    ctx = get_ctx("ConnectFour")
    pool, k, n_act = ctx.pool, len(IDS), 7
    if getattr(pool, "_guided_k", None) is not None:
        pool.guided_end()
    # a width outside 1 .. 32, through the wrapper and the C ABI, both forms; the refusals of the plain forms stay
    for width in (0, 33, -1):
        with pytest.raises(ValueError, match="guided_begin: width"):
            pool.guided_begin(IDS, 8, C_PUCT, 0, width)
        for device in (False, True):
            with pytest.raises(ValueError, match="guided_begin: width"):
                _raw_begin_wide(pool, IDS, 8, 0, width, C_PUCT, device)
    for call in (lambda: _raw_begin_wide(pool, IDS, 0, 0, 4, C_PUCT), lambda: _raw_begin_wide(pool, IDS, 8, 8, 4, C_PUCT),
                 lambda: _raw_begin_wide(pool, IDS, 8, 8193, 4, C_PUCT), lambda: _raw_begin_wide(pool, IDS, 8, 0, 4, -1.0),
                 lambda: _raw_begin_wide(pool, IDS[:0], 8, 0, 4, C_PUCT), lambda: _raw_begin_wide(pool, [70], 8, 0, 4, C_PUCT),
                 lambda: pool.guided_begin(IDS, 8, C_PUCT, 8, 4), lambda: pool.guided_begin(IDS, 0, C_PUCT, 0, 4)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match="no guided-search session"):  # none of them opened one
        pool.guided_end()
    env = envpool.make("ConnectFour-v1", "gymnasium", num_envs=4, seed=1)
    env.reset()
    for call in (lambda: env.guided_search(simulations=8, width=33), lambda: env.gumbel_search(simulations=8, width=2),
                 lambda: env.guided_search(simulations=8, policy="gumbel", width=2)):
        with pytest.raises(ValueError, match="width"):
            call()
    env.close()
    # a row count other than k W; a host reroot with a pending slot; none of them changes the session
    leaves = pool.guided_begin(IDS, 8, C_PUCT, 20, W)
    acts = np.full(k, 3, np.int32)
    calls = 0
    while (leaves[2] != 2).any():
        for rows in (k, k * W - 1, k * W + 1, 0):
            with pytest.raises(ValueError, match="guided_advance: priors and values of"):
                _raw_advance(pool, rows, n_act)
        with pytest.raises(ValueError, match="guided_advance"):
            pool.guided_advance(np.zeros((k, n_act), F), np.zeros(k, F))
        with pytest.raises(ValueError, match="round is not complete"):
            _raw_reroot(pool, acts, k, 8, W)
        with pytest.raises(ValueError, match="round is not complete"):
            pool.guided_reroot(acts, 8)
        leaves = pool.guided_advance(*evaluator(leaves[0], leaves[1]))
        calls += 1
    res = pool.guided_result()
    for call in (lambda: pool.guided_reroot(acts[:5], 8), lambda: _raw_reroot(pool, acts[:5], 5, 8, W),
                 lambda: _raw_reroot(pool, np.full(k * W, 3), k * W, 8, 1),
                 lambda: pool.guided_reroot(np.where(np.arange(k) == 3, 7, acts), 8),
                 lambda: pool.guided_reroot(acts, 20), lambda: _raw_reroot(pool, acts, k, 0, W)):
        with pytest.raises(ValueError, match="guided_reroot"):
            call()
    same(res, pool.guided_result())
    # later advances on a complete round change nothing, up to call number S; above it they are refused
    zeros = np.zeros((k, W, n_act), F), np.zeros((k, W), F)
    for _ in range(calls, 9):
        leaves = pool.guided_advance(*zeros)
        assert (leaves[2] == 2).all() and not leaves[0].any() and not leaves[1].any()
    same(res, pool.guided_result())
    with pytest.raises(ValueError, match="call number"):
        pool.guided_advance(*zeros)
    leaves = pool.guided_reroot(acts, 8)
    assert leaves[2].shape == (k, W) and (leaves[2][:, 1:] == 2).all()
    # a Gumbel session, and a plain one, replace it; the wide rows are then refused
    pool.gumbel_begin(np.zeros((k, n_act), F), IDS, 4)
    with pytest.raises(ValueError, match="gumbel|Gumbel"):
        pool.guided_advance(*zeros)
    pool.guided_begin(IDS, 8, C_PUCT)
    with pytest.raises(ValueError, match="guided_advance"):
        pool.guided_advance(*zeros)
    pool.guided_end()
    assert np.array_equal(pool.get_state(), ctx.st) and np.array_equal(pool.snapshot(), ctx.S)


def test_closing_a_pool_with_a_wide_session_open():
    pool = DevicePool("Othello", 8, seed=3)
    pool.reset(np.arange(8, dtype=np.int32))
    pool.recv_dict()
    leaves = pool.guided_begin(None, 16, C_PUCT, 40, 8)
    leaves = pool.guided_advance(*evaluator(leaves[0], leaves[1]))
    assert (leaves[2] == 0).sum() > 8
    pool.close()
    again = DevicePool("Othello", 8, seed=3)  # and a new pool works
    again.reset(np.arange(8, dtype=np.int32))
    again.recv_dict()
    first = again.guided_begin(None, 16, C_PUCT, 40, 8)
    same(again.guided_advance(*evaluator(first[0], first[1])), leaves)
    again.close()
