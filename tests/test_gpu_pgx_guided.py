"""PGX guided tree search on the MI355X: the stepwise kernels against the host harness of the same header fed the
pool's own hidden words and the same evaluator's numbers, for all four games, leaves after every call and results;
against the contract rebuilt from public calls only (restore, send / recv) with numpy scores; independence of id order,
repeated ids, sharding and of steps of the pool between advances; the device form with a torch model on the device;
the session's life cycle; the refusals.

The shape: a pool of 70 envs a few plies into their games with one env marked over, 11 ids out of order (11 blocks of
one wave), S = 24 simulations (Hex: S = 12)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import envpool_amd as envpool
from envpool_amd.core import native
from envpool_amd.core.device_pool import DevicePool
from pgx_guided_util import GuidedTree, Pos, stand_in
from pgx_util import ACTIONS, CODE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMES = ["TicTacToe", "ConnectFour", "Hex", "Othello"]
N, POOL_SEED, C_PUCT = 70, 11, 1.25
SIMS = {"TicTacToe": 24, "ConnectFour": 24, "Hex": 12, "Othello": 24}
PRE = {"TicTacToe": 4, "ConnectFour": 3, "Hex": 3, "Othello": 3}
OVER = 33  # the env marked over
IDS = np.array([41, 7, 69, OVER, 0, 64, 12, 63, 5, 50, 22], np.int32)  # 11 ids, not monotonic, both sides of lane 64
ALL = np.arange(N, dtype=np.int32)
F = np.float32


def legal_random(mask, rng):
    mask = np.asarray(mask, bool)
    return (rng.random(mask.shape) * mask + mask).argmax(1).astype(np.int32)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pgx_guided") / "libpgxguidedhost.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "cpu_harness", "pgx_guided_host.cpp"), "-o", out], check=True)
    lib = ctypes.CDLL(out)
    lib.pgx_guided_begin.restype = ctypes.c_void_p
    lib.pgx_guided_result.restype = None
    lib.pgx_guided_end.restype = None
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_session(lib, fam, st, simulations, c_puct, feed, result_at=()):
    """The harness on rows of get_state ([cur_step, done, hidden words]), fed feed[t] = (priors, values) at call t.
    Returns (the leaves before every call and after the last, the results after the calls `result_at`, the last)."""
    n_act, k = ACTIONS[fam], len(st)
    hid = np.ascontiguousarray(st[:, 2:], np.int32)
    done = np.ascontiguousarray(st[:, 1] != 0, np.uint8)
    h, w, c = {"TicTacToe": (3, 3, 2), "ConnectFour": (6, 7, 2), "Hex": (11, 11, 4), "Othello": (8, 8, 2)}[fam]
    obs, mask, status = np.full((k, h, w, c), 7, np.uint8), np.full((k, n_act), 7, np.uint8), np.full(k, 7, np.uint8)
    rc = ctypes.c_int(-9)
    s = lib.pgx_guided_begin(CODE[fam], k, _ptr(hid), _ptr(done), simulations, ctypes.c_float(c_puct), _ptr(obs),
                             _ptr(mask), _ptr(status), ctypes.byref(rc))
    assert rc.value == 0 and s

    def result():
        visits, values = np.full((k, n_act), -7, np.int32), np.full((k, n_act), -7, F)
        action, nodes = np.full(k, -7, np.int32), np.zeros(k, np.int32)
        lib.pgx_guided_result(ctypes.c_void_p(s), _ptr(visits), _ptr(values), _ptr(action), _ptr(nodes))
        return visits, values, action

    leaves, mids = [(obs.copy(), mask.copy(), status.copy())], {}
    for t in range(simulations + 1):
        priors, values = feed[t]
        priors, values = np.ascontiguousarray(priors, F), np.ascontiguousarray(values, F)
        assert lib.pgx_guided_advance(ctypes.c_void_p(s), _ptr(priors), _ptr(values), _ptr(obs), _ptr(mask),
                                      _ptr(status)) == 0
        leaves.append((obs.copy(), mask.copy(), status.copy()))
        if t in result_at:
            mids[t] = result()
    out = result()
    lib.pgx_guided_end(ctypes.c_void_p(s))
    return leaves, mids, out


def pool_session(pool, ids, simulations, c_puct, between=None, result_at=()):
    """A whole session of `pool` through the host forms with the stand-in evaluator.  Returns (the leaves before every
    call and after the last, the rows fed, the results after the calls `result_at`, the last); leaves the session
    open."""
    leaves, feed, mids = [pool.guided_begin(ids, simulations, c_puct)], [], {}
    for t in range(simulations + 1):
        obs, mask, _ = leaves[-1]
        feed.append(stand_in(obs, mask))
        if between is not None:
            between(t)
        leaves.append(pool.guided_advance(*feed[-1]))
        if t in result_at:
            mids[t] = pool.guided_result()
    return leaves, feed, mids, pool.guided_result()


def same(a, b):
    """Two tuples of arrays, bit for bit (floats by their bits)."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape, (x.shape, y.shape)
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), np.ascontiguousarray(y, F).view(np.uint32)
        assert np.array_equal(x, y)


def rolled(fam, step):
    """PRE[fam] seeded random legal plies of every env through `step(actions) -> legal mask`."""
    rng = np.random.default_rng(2)
    mask = step(None)
    for _ in range(PRE[fam]):
        mask = step(legal_random(mask, rng))
    return mask


class Ctx:
    """One pool per game, a few plies in, env OVER marked over, with its state, snapshot and one whole session."""

    def __init__(self, fam):
        self.fam = fam
        self.pool = pool = DevicePool(fam, N, seed=POOL_SEED)

        def step(act):
            if act is None:
                pool.reset(ALL)
            else:
                pool.send(ALL, act)
            out = pool.recv_dict()
            assert np.array_equal(out["info:env_id"], ALL)
            self.out0 = {k: np.asarray(v).copy() for k, v in out.items()}
            return out["info:legal_action_mask"]

        rolled(fam, step)
        row = pool.get_state([OVER])
        row[0, 1] = 1.0
        pool.set_state(row, [OVER])
        self.st = pool.get_state()
        self.S = pool.snapshot()
        self.mid = SIMS[fam] // 2
        self.leaves, self.feed, self.mids, self.got = pool_session(pool, IDS, SIMS[fam], C_PUCT,
                                                                   result_at=(self.mid,))


_ctx = {}


def get_ctx(fam):
    if fam not in _ctx:
        _ctx[fam] = Ctx(fam)
    return _ctx[fam]


@pytest.fixture(scope="module", params=GAMES)
def ctx(request):
    return get_ctx(request.param)


def test_kernels_equal_the_host_harness_and_change_nothing(ctx, harness):
    fam, n_act, sims = ctx.fam, ACTIONS[ctx.fam], SIMS[ctx.fam]
    visits, values, action = ctx.got
    assert visits.shape == (len(IDS), n_act) and visits.dtype == np.int32
    assert values.shape == (len(IDS), n_act) and values.dtype == np.float32
    assert action.shape == (len(IDS),) and action.dtype == np.int32
    obs, mask, status = ctx.leaves[0]
    assert obs.dtype == np.bool_ and mask.dtype == np.bool_ and status.dtype == np.uint8
    assert obs.shape[0] == len(IDS) and mask.shape == (len(IDS), n_act) and status.shape == (len(IDS),)
    assert np.array_equal(ctx.pool.get_state(), ctx.st)
    assert np.array_equal(ctx.pool.snapshot(), ctx.S)
    over = ctx.st[IDS, 1] != 0
    assert over[list(IDS).index(OVER)] and not over.all()
    assert len(np.unique(ctx.st[IDS][:, 2:], axis=0)) > len(IDS) // 2  # the positions differ
    leaves, mids, want = host_session(harness, fam, ctx.st[IDS], sims, C_PUCT, ctx.feed, result_at=(ctx.mid,))
    assert len(ctx.leaves) == sims + 2
    for t, (g, w) in enumerate(zip(ctx.leaves, leaves)):
        for x, y in zip(g, w):
            assert np.array_equal(x.view(np.uint8), y), (fam, t)  # (bool bytes are 0 / 1)
    same(ctx.got, want)
    same(ctx.mids[ctx.mid], mids[ctx.mid])  # result() mid-session
    assert (ctx.mids[ctx.mid][0][~over].sum(1) == ctx.mid).all()
    # the first leaves are the rows the last step returned for the seat to move
    mover = ctx.out0["info:current_player"]
    rows = ctx.out0["obs"].reshape((N, 2) + obs.shape[1:])
    for j, e in enumerate(IDS):
        if e == OVER:
            assert status[j] == 2 and not obs[j].any() and not mask[j].any()
        else:
            assert status[j] == 0
            assert np.array_equal(obs[j], rows[e, mover[e]]) and np.array_equal(mask[j],
                                                                                ctx.out0["info:legal_action_mask"][e])
    last = ctx.leaves[-1]
    assert (last[2] == 2).all() and not last[0].any() and not last[1].any()
    assert (action[over] == -1).all() and not visits[over].any() and not values[over].any()
    assert (visits[~over].sum(1) == sims).all() and (action[~over] >= 0).all()
    seen = np.concatenate([lv[2] for lv in ctx.leaves])
    assert 0 in seen and 2 in seen and (fam != "TicTacToe" or 1 in seen)
    if fam == "Hex":
        assert visits[:, 64:].sum() > 0  # the second action slot of a lane
    # c_puct = 0 and fewer roots: still the harness
    lv, feed, _, got = pool_session(ctx.pool, IDS[:5], sims, 0.0)
    lv2, _, want = host_session(harness, fam, ctx.st[IDS[:5]], sims, 0.0, feed)
    same(got, want)
    for g, w in zip(lv, lv2):
        for x, y in zip(g, w):
            assert np.array_equal(x.view(np.uint8), y)


def test_steps_of_the_pool_between_advances_change_nothing(ctx):
    """The session works on its own copies: the pool is stepped (and searched, which uses the side scratch) between
    the advances, and the session gives the leaves and results it gave when the pool stood still."""
    pool, fam = ctx.pool, ctx.fam
    rng = np.random.default_rng(9)
    state = {"mask": ctx.out0["info:legal_action_mask"]}

    def between(t):
        if t % 3 == 1:
            pool.send(ALL, legal_random(state["mask"], rng))
            state["mask"] = pool.recv_dict()["info:legal_action_mask"]
        if t == 2:
            pool.search(IDS[:3], 4, 2, C_PUCT, 0, 1)
            pool.get_state()

    leaves, _, _, got = pool_session(pool, IDS, SIMS[fam], C_PUCT, between=between)
    assert not np.array_equal(pool.get_state(), ctx.st)  # the pool did move
    same(got, ctx.got)
    for g, w in zip(leaves, ctx.leaves):
        same(g, w)
    pool.restore(ctx.S)
    assert np.array_equal(pool.get_state(), ctx.st)


@pytest.mark.parametrize("fam", ["TicTacToe", "Othello"])
def test_search_rebuilt_from_public_calls(fam):
    """The trees in Python (pgx_guided_util.py); a node is a single-env snapshot; expansion is restore + send / recv +
    snapshot in env e, and the obs and mask of a leaf are what that recv returned for the current player."""
    ctx = get_ctx(fam)
    pool = ctx.pool
    sims, roots = 16, [int(i) for i in IDS if i != OVER][:4]
    obs_shape = ctx.leaves[0][0].shape[1:]
    trees = []
    for e in roots:
        ids = np.array([e], np.int32)

        def expand(pos, a, ids=ids):
            pool.restore(pos.key, ids)
            pool.send(ids, np.array([a], np.int32))
            out = pool.recv_dict()
            rw = np.asarray(out["reward"]).reshape(2)
            assert rw[0] == -rw[1]
            mover = int(out["info:current_player"][0])
            new = Pos(mask=np.asarray(out["info:legal_action_mask"], bool).reshape(-1), done=bool(out["done"][0]),
                      mover=mover, obs=np.asarray(out["obs"], bool).reshape((2,) + obs_shape)[mover],
                      key=pool.snapshot(ids))
            return new, int(rw[0])

        mover = int(ctx.out0["info:current_player"][e])
        root = Pos(mask=np.asarray(ctx.out0["info:legal_action_mask"][e], bool), done=False, mover=mover,
                   obs=np.asarray(ctx.out0["obs"], bool).reshape((N, 2) + obs_shape)[e, mover], key=pool.snapshot(ids))
        trees.append(GuidedTree(root, False, expand, sims, C_PUCT))
    leaves = pool.guided_begin(np.array(roots, np.int32), sims, C_PUCT)
    for t in range(sims + 1):
        for j, tree in enumerate(trees):
            want = tree.leaf()
            assert leaves[2][j] == want[2], (fam, t, j)
            assert np.array_equal(leaves[0][j], want[0]) and np.array_equal(leaves[1][j], want[1]), (fam, t, j)
        priors, values = stand_in(leaves[0], leaves[1])
        leaves = pool.guided_advance(priors, values)
        for j, tree in enumerate(trees):
            tree.advance(priors[j], values[j])
    got = pool.guided_result()
    for j, tree in enumerate(trees):
        want = tree.result()
        assert np.array_equal(got[0][j], want[0]), (fam, j)
        assert np.array_equal(got[1][j].view(np.uint32), want[1].view(np.uint32)), (fam, j)
        assert got[2][j] == want[2]
    pool.restore(ctx.S)
    assert np.array_equal(pool.get_state(), ctx.st)


def test_id_order_and_repeated_ids(ctx):
    pool, fam = ctx.pool, ctx.fam
    perm = np.random.default_rng(4).permutation(len(IDS))
    leaves, _, _, got = pool_session(pool, IDS[perm], SIMS[fam], C_PUCT)
    same(got, [w[perm] for w in ctx.got])
    for g, w in zip(leaves, ctx.leaves):
        same(g, [x[perm] for x in w])
    pick = [1, 1, 0, 4, 1]
    _, _, _, twice = pool_session(pool, IDS[pick], SIMS[fam], C_PUCT)  # ids may repeat
    same(twice, [w[pick] for w in ctx.got])
    _, _, _, whole = pool_session(pool, None, 4, C_PUCT)  # the whole pool: the identity id table, 70 blocks
    _, _, _, part = pool_session(pool, IDS, 4, C_PUCT)
    same([w[IDS] for w in whole], part)
    assert np.array_equal(pool.get_state(), ctx.st) and np.array_equal(pool.snapshot(), ctx.S)


@pytest.mark.parametrize("fam", GAMES)
def test_sharded_pool_equals_the_unsharded(fam):
    """device=[0, 0]: two shards, the second with env_id_offset 35, one session in each; rows in request order."""
    results = []
    for device in ([0, 0], 0):
        env = envpool.make(f"{fam}-v1", "gymnasium", num_envs=N, device=device, seed=POOL_SEED)

        def step(act):
            if act is None:
                _, info = env.reset()
            else:
                _, _, _, _, info = env.step(act)
            return info["legal_action_mask"]

        rolled(fam, step)
        gs = env.guided_search(IDS, simulations=SIMS[fam], c_puct=C_PUCT)
        first = gs.leaves
        calls = []

        def evaluate(obs, mask, status):
            calls.append(status.copy())
            return stand_in(obs, mask)

        out = gs.run(evaluate)
        assert out._fields == ("visits", "values", "action") and len(calls) == SIMS[fam] + 1
        results.append((out, first, calls))
        env.close()
    assert (IDS < N // 2).any() and (IDS >= N // 2).any() and (np.diff(IDS // (N // 2)) != 0).sum() > 2
    same(results[0][0], results[1][0])
    same(results[0][1], results[1][1])
    same(results[0][2], results[1][2])
    assert results[0][0].visits.sum() == len(IDS) * SIMS[fam]


def test_device_form_with_a_model_on_the_device(ctx):
    """guided_search_device with a small seeded torch model evaluated on the device; the same search through the host
    form, fed the priors and values the model gave, copied back to the host."""
    import torch

    from envpool_amd.torch_interop import guided_search_device

    pool, fam, n_act = ctx.pool, ctx.fam, ACTIONS[ctx.fam]
    dev = torch.device("cuda", pool.device)
    n_obs = int(np.prod(ctx.leaves[0][0].shape[1:]))
    gen = torch.Generator().manual_seed(3)
    w_p = (torch.randn((n_obs, n_act), generator=gen) * 0.3).to(dev)
    w_v = (torch.randn((n_obs,), generator=gen) * 0.2).to(dev)
    fed, seen = [], []

    def model(obs, mask):
        x = obs.reshape(obs.shape[0], -1).float()
        return torch.softmax(x @ w_p, dim=1) * mask.float(), torch.tanh(x @ w_v)

    def evaluate(obs, mask, status):
        assert obs.is_cuda and obs.dtype == torch.bool and mask.dtype == torch.bool and status.dtype == torch.uint8
        priors, values = model(obs, mask)
        fed.append((priors.cpu().numpy(), values.cpu().numpy()))
        seen.append((obs.cpu().numpy(), mask.cpu().numpy(), status.cpu().numpy()))
        return priors, values

    dev_out = guided_search_device(pool, evaluate, IDS, SIMS[fam], C_PUCT)
    assert all(t.is_cuda for t in dev_out)
    assert dev_out[0].dtype == torch.int32 and dev_out[1].dtype == torch.float32 and dev_out[2].dtype == torch.int32
    assert len(fed) == SIMS[fam] + 1
    with pytest.raises(ValueError, match="no guided-search session"):  # it closed its session
        pool.guided_end()
    leaves = [pool.guided_begin(IDS, SIMS[fam], C_PUCT)]
    for priors, values in fed:
        leaves.append(pool.guided_advance(priors, values))
    same([t.cpu().numpy() for t in dev_out], pool.guided_result())
    for g, w in zip(seen, leaves):
        same(g, w)
    assert len(np.unique(np.concatenate([f[1] for f in fed]))) > SIMS[fam]  # the model did look at the leaves
    # what the kernel makes of entries outside their range: zeros, as the contract's clean / cleanv say
    junk = [float("nan"), float("inf"), -1.0]

    def spoiled(zeros):
        count = [0]

        def run(obs, mask, status):
            priors, values = model(obs, mask)
            t, count[0] = count[0], count[0] + 1
            priors[:, t % n_act] = 0.0 if zeros else junk[t % 3]
            if t % 2:
                values = torch.zeros_like(values) if zeros else (values + 1.5) * float("inf")
            return priors, values

        return [t.cpu().numpy() for t in guided_search_device(pool, run, IDS, SIMS[fam], C_PUCT)]

    a, b = spoiled(False), spoiled(True)
    assert np.isfinite(a[1]).all()
    same(a, b)
    assert not np.array_equal(a[1], dev_out[1].cpu().numpy())
    assert np.array_equal(pool.get_state(), ctx.st) and np.array_equal(pool.snapshot(), ctx.S)


def test_session_life_cycle():
    ctx = get_ctx("ConnectFour")
    pool = ctx.pool
    pool_session(pool, IDS, 6, C_PUCT)
    # a second begin replaces the session: other roots, another S
    leaves = pool.guided_begin(IDS[:4], 3, C_PUCT)
    assert leaves[0].shape[0] == 4
    with pytest.raises(ValueError, match="guided_advance"):
        pool.guided_advance(*stand_in(*ctx.leaves[0][:2]))  # rows of the replaced session
    _, _, _, got = pool_session(pool, IDS[:4], 3, C_PUCT)
    assert (got[0].sum(1) == np.where(ctx.st[IDS[:4], 1] != 0, 0, 3)).all()
    pool.guided_end()
    for call in (pool.guided_end, pool.guided_result, lambda: pool.guided_advance(*stand_in(*leaves[:2]))):
        with pytest.raises(ValueError, match="no guided-search session"):
            call()
    assert np.array_equal(pool.get_state(), ctx.st)
    # the env classes: close() ends the session, and a pool can be closed with a session open
    env = envpool.make("TicTacToe-v1", "gymnasium", num_envs=8, seed=1)
    env.reset()
    gs = env.guided_search(simulations=4)
    assert gs.leaves[2].tolist() == [0] * 8 and gs.leaves[1].all()
    gs.advance(*stand_in(*gs.leaves[:2]))
    assert gs.result().visits.sum() == 0  # the first advance backs nothing up
    gs.advance(*stand_in(*gs.leaves[:2]))
    assert (gs.result().visits.sum(1) == 1).all()
    gs.close()
    with pytest.raises(ValueError, match="closed"):
        gs.result()
    gs = env.guided_search([3, 1], simulations=4)
    gs.advance(*stand_in(*gs.leaves[:2]))
    env.close()
    other = DevicePool("Othello", 4, seed=1)
    other.reset(np.arange(4, dtype=np.int32))
    other.recv_dict()
    other.guided_begin(None, 8, C_PUCT)
    other.close()


def _raw_begin(pool, ids, simulations, c_puct):
    """epa_guided_begin itself, past the wrapper's checks."""
    ids = np.ascontiguousarray(ids, np.int32)
    k = max(len(ids), 1)
    h, w, c, a = pool.guided_shape()
    obs, mask, status = np.zeros((k, h, w, c), np.uint8), np.zeros((k, a), np.uint8), np.zeros(k, np.uint8)
    native.check(pool._lib.epa_guided_begin(pool._h, ids.ctypes.data, len(ids), simulations, ctypes.c_float(c_puct),
                                            obs.ctypes.data, mask.ctypes.data, status.ctypes.data))
    return obs, mask, status


def _raw_advance(pool, priors, values, k):
    h, w, c, a = pool.guided_shape()
    n = max(k, 1)
    obs, mask, status = np.zeros((n, h, w, c), np.uint8), np.zeros((n, a), np.uint8), np.zeros(n, np.uint8)
    native.check(pool._lib.epa_guided_advance(pool._h, priors.ctypes.data, values.ctypes.data, k, obs.ctypes.data,
                                              mask.ctypes.data, status.ctypes.data))
    return obs, mask, status


def test_errors():
    cart = DevicePool("CartPole", 4, seed=1)
    from envpool_amd.torch_interop import guided_search_device

    for call in (lambda: cart.guided_begin(None), lambda: guided_search_device(cart, None), cart.guided_end,
                 lambda: native.check(cart._lib.epa_guided_result(cart._h, None, None, None))):
        with pytest.raises(RuntimeError, match="guided search not implemented"):
            call()
    buf = np.zeros(64, np.int32)
    with pytest.raises(RuntimeError, match="guided search not implemented"):
        native.check(cart._lib.epa_guided_begin(cart._h, buf.ctypes.data, 2, 8, ctypes.c_float(1.0), buf.ctypes.data,
                                                buf.ctypes.data, buf.ctypes.data))
    cart.close()
    ctx = get_ctx("TicTacToe")
    pool = ctx.pool
    if getattr(pool, "_guided_k", None) is not None:
        pool.guided_end()
    zeros = (np.zeros((len(IDS), 9), F), np.zeros(len(IDS), F))
    # without a session, through the wrapper and the C ABI
    for call in (lambda: pool.guided_advance(*zeros), pool.guided_result, pool.guided_end,
                 lambda: _raw_advance(pool, zeros[0], zeros[1], len(IDS)),
                 lambda: native.check(pool._lib.epa_guided_result(pool._h, zeros[0].ctypes.data, zeros[0].ctypes.data,
                                                                  zeros[1].ctypes.data))):
        with pytest.raises(ValueError, match="no guided-search session"):
            call()
    bad = [dict(simulations=0), dict(simulations=4097), dict(c_puct=-1.0), dict(c_puct=float("nan")),
           dict(c_puct=float("inf"))]
    base = dict(simulations=8, c_puct=C_PUCT)
    for kw in bad:
        a = {**base, **kw}
        with pytest.raises(ValueError, match="guided_begin"):
            pool.guided_begin(IDS, **a)
        with pytest.raises(ValueError, match="guided_begin"):
            _raw_begin(pool, IDS, a["simulations"], a["c_puct"])
    # the id checks of search, through both
    for ids in ([0, N], [-1], []):
        with pytest.raises(ValueError):
            pool.guided_begin(np.array(ids, np.int32), **base)
        with pytest.raises(ValueError):
            _raw_begin(pool, ids, 8, C_PUCT)
    with pytest.raises(ValueError, match="exceeds num_envs"):
        pool.guided_begin(np.zeros(N + 1, np.int32), **base)
    with pytest.raises(ValueError, match="exceeds num_envs"):
        _raw_begin(pool, np.zeros(N + 1, np.int32), 8, C_PUCT)
    with pytest.raises(ValueError, match="no guided-search session"):  # none of them opened one
        pool.guided_end()
    # rows: their number, and numbers the host forms refuse
    leaves = pool.guided_begin(IDS, 2, C_PUCT)
    good = stand_in(leaves[0], leaves[1])
    for priors, values in ((good[0][:5], good[1][:5]), (good[0], good[1][:5]), (good[0][:, :8], good[1])):
        with pytest.raises(ValueError, match="guided_advance"):
            pool.guided_advance(priors, values)
    with pytest.raises(ValueError, match="guided_advance"):
        _raw_advance(pool, np.ascontiguousarray(good[0][:5]), np.ascontiguousarray(good[1][:5]), 5)
    for i, x in ((0, np.nan), (0, np.inf), (0, -0.5), (1, 2.0), (1, np.nan)):
        rows = [good[0].copy(), good[1].copy()]
        rows[i].reshape(-1)[3] = x
        with pytest.raises(ValueError, match="guided_advance"):
            pool.guided_advance(*rows)
        with pytest.raises(ValueError, match="guided_advance"):
            _raw_advance(pool, rows[0], rows[1], len(IDS))
    # none of the refused calls counted: S + 1 = 3 advances pass, the fourth is a call number above S
    for _ in range(3):
        leaves = pool.guided_advance(*stand_in(leaves[0], leaves[1]))
    with pytest.raises(ValueError, match="above simulations"):
        pool.guided_advance(*good)
    with pytest.raises(ValueError, match="above simulations"):
        _raw_advance(pool, good[0], good[1], len(IDS))
    over = ctx.st[IDS, 1] != 0
    assert (pool.guided_result()[0].sum(1) == np.where(over, 0, 2)).all()
    pool.guided_end()
    assert np.array_equal(pool.get_state(), ctx.st) and np.array_equal(pool.snapshot(), ctx.S)


def test_trees_above_2_gib_are_refused(harness):
    """Hex with 4096 simulations: 4097 nodes per root; the message names the most roots that fit."""
    node = harness.pgx_guided_node_bytes(CODE["Hex"])
    fits = 2**31 // (4097 * node)
    pool = DevicePool("Hex", fits + 8, seed=1)
    pool.reset(np.arange(fits + 8, dtype=np.int32))
    pool.recv_dict()
    st = pool.get_state()
    with pytest.raises(ValueError, match=f"at most {fits} roots"):
        pool.guided_begin(np.arange(fits + 1, dtype=np.int32), 4096, C_PUCT)
    with pytest.raises(ValueError, match=f"at most {fits} roots"):
        _raw_begin(pool, np.arange(fits + 1, dtype=np.int32), 4096, C_PUCT)
    assert np.array_equal(pool.get_state(), st)
    _, _, _, out = pool_session(pool, np.arange(3, dtype=np.int32), 8, C_PUCT)  # and the pool still searches
    assert (out[0].sum(1) == 8).all()
    pool.close()


def teardown_module(module):
    for c in _ctx.values():
        c.pool.close()
    _ctx.clear()
