"""PGX Gumbel search on the MI355X: the stepwise kernels against the host harness of the same header fed the same
positions and the same evaluator's numbers, for all four games, leaves after every advance and all four result arrays,
bit for bit; independence of id order, sharding and of steps of the pool between advances; the device form with a
torch model on the device; the session's life cycle shared with the PUCT policy; minimax-optimal moves from exact
values; the refusals.

The shape: a pool of 8 envs set to chosen positions (mid-game fixture rows, a root one ply from the end, a root that is
over, Othello's forced pass, Hex with the swap legal), 8 ids out of order (8 blocks of one wave), S in {1, 16},
m in {2, 16}."""
import ctypes

import numpy as np
import pytest

import envpool_amd as envpool
from envpool_amd.core import native
from envpool_amd.core.device_pool import DevicePool
from pgx_gumbel_util import gumbel_noise, stand_in_logits, wild_logits
from pgx_util import ACTIONS
from test_pgx_guided_host import Replayed, mid_row
from test_pgx_gumbel_host import (HostSession, _build, exact_evaluator, minimax, optimal_moves, tictactoe_cells,
                                  two_ply_roots)

pytestmark = pytest.mark.gpu

GAMES = ["TicTacToe", "ConnectFour", "Hex", "Othello"]
N = 8
IDS = np.array([5, 2, 7, 0, 3, 6, 1, 4], np.int32)
ALL = np.arange(N, dtype=np.int32)
F = np.float32


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pgx_gumbel_gpu")
    gumbel = _build(tmp, "pgx_gumbel_host.cpp", "libpgxgumbelhost.so")
    gumbel.pgx_gumbel_begin.restype = ctypes.c_void_p
    gumbel.pgx_gumbel_result.restype = None
    gumbel.pgx_gumbel_end.restype = None
    return _build(tmp, "pgx_host.cpp", "libpgxhost.so"), gumbel


def same(a, b):
    """Two tuples of arrays, bit for bit (floats by their bits; bool bytes are 0 / 1)."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.shape == y.shape, (x.shape, y.shape)
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), np.ascontiguousarray(y, F).view(np.uint32)
        elif x.dtype == np.bool_ or y.dtype == np.bool_:
            x, y = x.view(np.uint8), y.view(np.uint8)
        assert np.array_equal(x, y)


def forced_pass(game_):
    rng = np.random.default_rng(5)
    for _ in range(400):
        seq = []
        pos, _ = game_.at(seq)
        while not pos.done:
            if pos.mask[64]:
                return pos
            seq.append(int(rng.choice(np.flatnonzero(pos.mask))))
            pos, _ = game_.at(seq)
    raise AssertionError("no forced pass found")


def roots_of(libs, fam):
    """The 8 positions of the game's pool, env e = roots[e]."""
    tid = f"{fam}-v1"
    cols = [Replayed(libs, tid, column=c) for c in range(4)]
    mids = [g.fixture_row(mid_row(g.g, g.column)) for g in cols]
    first = cols[0]
    over = first.fixture_row(int(np.flatnonzero(first.g["done"][:, 0])[0]))
    assert over.done and not any(p.done for p in mids)
    if fam == "TicTacToe":
        extra = [first.at([0, 1, 2, 4, 3, 5])[0], first.at([4, 0])[0], first.at([])[0]]  # one ply from the end
    elif fam == "Othello":
        extra = [forced_pass(first), first.at([])[0], cols[1].fixture_row(mid_row(cols[1].g, 1) + 4)]
    elif fam == "Hex":
        extra = [first.at([60])[0], first.at([])[0], cols[1].fixture_row(mid_row(cols[1].g, 1) + 6)]  # the swap
    else:
        extra = [first.at([3, 3, 3])[0], first.at([])[0], cols[1].fixture_row(mid_row(cols[1].g, 1) + 3)]
    assert not any(p.done for p in extra)
    return mids + [over] + extra


class Ctx:
    """One pool per game with its 8 envs set to the roots, its state and snapshot."""

    def __init__(self, libs, fam):
        self.fam, self.tid, self.n_act = fam, f"{fam}-v1", ACTIONS[fam]
        self.roots = roots_of(libs, fam)
        self.pool = pool = DevicePool(fam, N, seed=11)
        pool.reset(ALL)
        pool.recv_dict()
        rows = np.array([[len(p.key[0]), float(p.done)] + p.key[1].tolist() for p in self.roots], np.float64)
        pool.set_state(rows, ALL)
        self.st = pool.get_state()
        self.S = pool.snapshot()

    def poss(self, ids):
        return [self.roots[int(e)] for e in ids]


_ctx = {}


def get_ctx(libs, fam):
    if fam not in _ctx:
        _ctx[fam] = Ctx(libs, fam)
    return _ctx[fam]


@pytest.fixture(scope="module", params=GAMES)
def ctx(request, libs):
    return get_ctx(libs, request.param)


def pool_session(pool, ids, simulations, considered, gumbel, evaluate=stand_in_logits, between=None):
    """A whole session of `pool` through the host forms.  Returns (the leaves before every call and after the last,
    the rows fed, the result after every call); leaves the session open."""
    leaves, feed, results = [pool.gumbel_begin(gumbel, ids, simulations, considered)], [], []
    for t in range(simulations + 1):
        obs, mask, _ = leaves[-1]
        feed.append(evaluate(obs, mask))
        if between is not None:
            between(t)
        leaves.append(pool.gumbel_advance(*feed[-1]))
        results.append(pool.gumbel_result())
    return leaves, feed, results


def host_session(libs, ctx, ids, simulations, considered, gumbel, feed):
    host = HostSession(libs, ctx.tid, ctx.poss(ids), simulations, considered, gumbel)
    leaves, results = [host.leaves()], []
    for t in range(simulations + 1):
        assert host.advance(*feed[t]) == 0
        leaves.append(host.leaves())
        results.append(host.result()[:4])
    host.close()
    return leaves, results


@pytest.mark.parametrize("considered", [2, 16])
@pytest.mark.parametrize("simulations", [1, 16])
def test_kernels_equal_the_host_harness_and_change_nothing(ctx, libs, simulations, considered):
    pool = ctx.pool
    for evaluate, gumbel in ((stand_in_logits, gumbel_noise(3, N, ctx.n_act)), (wild_logits, np.zeros((N, ctx.n_act), F))):
        leaves, feed, results = pool_session(pool, IDS, simulations, considered, gumbel, evaluate)
        want_leaves, want = host_session(libs, ctx, IDS, simulations, considered, gumbel, feed)
        assert len(leaves) == simulations + 2
        for t, (g, w) in enumerate(zip(leaves, want_leaves)):
            assert g[0].dtype == np.bool_ and g[1].dtype == np.bool_ and g[2].dtype == np.uint8
            same(g, w)
        for t, (g, w) in enumerate(zip(results, want)):
            same(g, w)
        visits, values, action, weights = results[-1]
        assert visits.dtype == np.int32 and values.dtype == F and action.dtype == np.int32 and weights.dtype == F
        over = np.array([p.done for p in ctx.poss(IDS)])
        assert over.sum() == 1 and (action[over] == -1).all() and not weights[over].any()
        assert (visits[~over].sum(1) == simulations).all() and (action[~over] >= 0).all()
        assert np.allclose(weights[~over].sum(1, dtype=np.float64), 1, atol=1e-6)
        seen = np.concatenate([lv[2] for lv in leaves])
        assert 0 in seen and 2 in seen and (ctx.fam != "TicTacToe" or simulations == 1 or 1 in seen)
        assert (leaves[-1][2] == 2).all() and not leaves[-1][0].any()
    pool.guided_end()
    assert np.array_equal(pool.get_state(), ctx.st) and np.array_equal(pool.snapshot(), ctx.S)  # nothing changed


def test_rows_follow_their_ids(ctx):
    pool = ctx.pool
    gumbel = gumbel_noise(5, N, ctx.n_act)
    order = np.argsort(IDS)
    a = pool_session(pool, IDS, 16, 4, gumbel)
    b = pool_session(pool, IDS[order], 16, 4, gumbel[order])
    for x, y in zip(a[0], b[0]):
        same([v[order] for v in x], y)
    same([v[order] for v in a[2][-1]], b[2][-1])
    pool.guided_end()


def test_steps_of_the_pool_between_advances_change_nothing(ctx):
    pool = ctx.pool
    gumbel = gumbel_noise(6, N, ctx.n_act)
    plain = pool_session(pool, IDS, 16, 4, gumbel)

    def between(t):
        if t % 3 == 1:
            mask = np.array([p.mask for p in ctx.roots])
            pool.send(ALL, mask.argmax(1).astype(np.int32))  # (the env that is over resets)
            pool.recv_dict()
            pool.restore(ctx.S)
        if t == 2:
            pool.search(IDS[:3], 4, 2, 1.25, 0, 1)  # (the side scratch is not the session's memory)

    moved = pool_session(pool, IDS, 16, 4, gumbel, between=between)
    for x, y in zip(plain[0], moved[0]):
        same(x, y)
    same(plain[2][-1], moved[2][-1])
    pool.guided_end()
    pool.restore(ctx.S)
    assert np.array_equal(pool.get_state(), ctx.st)


def legal_random(mask, rng):
    mask = np.asarray(mask, bool)
    return (rng.random(mask.shape) * mask + mask).argmax(1).astype(np.int32)


@pytest.mark.parametrize("fam", ["ConnectFour", "Hex"])
def test_sharded_pool_equals_the_unsharded(fam):
    """device=[0, 0]: two shards of 4 envs, one session in each; gumbel rows follow their ids, result rows come back
    in request order."""
    gumbel = gumbel_noise(8, len(IDS), ACTIONS[fam])
    results = []
    for device in ([0, 0], 0):
        env = envpool.make(f"{fam}-v1", "gymnasium", num_envs=N, device=device, seed=11)
        rng = np.random.default_rng(2)
        _, info = env.reset()
        for _ in range(3):
            _, _, _, _, info = env.step(legal_random(info["legal_action_mask"], rng))
        gs = env.guided_search(IDS, simulations=16, policy="gumbel", max_considered=4, gumbel=gumbel)
        first, calls = gs.leaves, []

        def evaluate(obs, mask, status):
            calls.append(status.copy())
            return stand_in_logits(obs, mask)

        out = gs.run(evaluate)
        assert out._fields == ("visits", "values", "action", "weights") and len(calls) == 17
        results.append((out, first, calls))
        env.close()
    same(results[0][0], results[1][0])
    same(results[0][1], results[1][1])
    same(results[0][2], results[1][2])
    assert results[0][0].visits.sum() == len(IDS) * 16


def test_device_form_with_a_model_on_the_device(ctx):
    import torch

    from envpool_amd.torch_interop import gumbel_search_device

    pool, n_act = ctx.pool, ctx.n_act
    dev = torch.device("cuda", pool.device)
    n_obs = int(np.prod(ctx.roots[0].obs.shape))
    gen = torch.Generator().manual_seed(3)
    w_p = (torch.randn((n_obs, n_act), generator=gen) * 0.7).to(dev)
    w_v = (torch.randn((n_obs,), generator=gen) * 0.2).to(dev)
    gumbel = gumbel_noise(9, N, n_act)
    fed, seen = [], []

    def evaluate(obs, mask, status):
        assert obs.is_cuda and obs.dtype == torch.bool and mask.dtype == torch.bool and status.dtype == torch.uint8
        x = obs.reshape(obs.shape[0], -1).float()
        logits, values = x @ w_p, torch.tanh(x @ w_v)
        fed.append((logits.cpu().numpy(), values.cpu().numpy()))
        seen.append((obs.cpu().numpy(), mask.cpu().numpy(), status.cpu().numpy()))
        return logits, values

    out = gumbel_search_device(pool, evaluate, IDS, 16, 4, torch.from_numpy(gumbel).to(dev))
    assert all(t.is_cuda for t in out) and [t.dtype for t in out] == [torch.int32, torch.float32, torch.int32,
                                                                       torch.float32]
    with pytest.raises(ValueError, match="no guided-search session"):  # it closed its session
        pool.guided_end()
    leaves = [pool.gumbel_begin(gumbel, IDS, 16, 4)]
    for logits, values in fed:
        leaves.append(pool.gumbel_advance(logits, values))
    same([t.cpu().numpy() for t in out], pool.gumbel_result())
    for g, w in zip(seen, leaves):
        same(g, w)
    pool.guided_end()
    # torch draws the noise when none is given: seeded draws repeat
    a = gumbel_search_device(pool, evaluate, IDS, 4, 4, seed=1)
    b = gumbel_search_device(pool, evaluate, IDS, 4, 4, seed=1)
    same([t.cpu().numpy() for t in a], [t.cpu().numpy() for t in b])
    assert np.array_equal(pool.get_state(), ctx.st) and np.array_equal(pool.snapshot(), ctx.S)


def test_one_session_of_either_policy(libs):
    """A Gumbel begin releases an open PUCT session and the reverse; the other policy's advance and result are refused
    by the wrappers and by the C ABI; end, the next begin and the pool's destructor release the memory."""
    ctx = get_ctx(libs, "ConnectFour")
    pool, n_act = ctx.pool, ctx.n_act
    zeros = (np.zeros((4, n_act), F), np.zeros(4, F))
    out4 = (np.zeros((4, n_act), np.int32), np.zeros((4, n_act), F), np.zeros(4, np.int32), np.zeros((4, n_act), F))
    leaf = (np.zeros((4, 6, 7, 2), np.uint8), np.zeros((4, n_act), np.uint8), np.zeros(4, np.uint8))

    def raw(fn, *arrays, k=None):
        args = [a.ctypes.data for a in arrays]
        if k is not None:
            args.insert(2, k)
        native.check(getattr(pool._lib, fn)(pool._h, *args))

    pool.guided_begin(IDS[:4], 4, 1.25)
    pool.gumbel_begin(np.zeros((4, n_act), F), IDS[:4], 4, 2)  # releases the PUCT session
    for call in (lambda: pool.guided_advance(*zeros), pool.guided_result,
                 lambda: raw("epa_guided_advance", *zeros, *leaf, k=4), lambda: raw("epa_guided_result", *out4[:3])):
        with pytest.raises(ValueError, match="Gumbel search: use gumbel_"):
            call()
    pool.gumbel_advance(*zeros)
    pool.guided_begin(IDS[:4], 4, 1.25)  # and the reverse
    for call in (lambda: pool.gumbel_advance(*zeros), pool.gumbel_result,
                 lambda: raw("epa_gumbel_advance", *zeros, *leaf, k=4), lambda: raw("epa_gumbel_result", *out4)):
        with pytest.raises(ValueError, match="PUCT guided search: use guided_"):
            call()
    pool.guided_advance(np.full((4, n_act), 0.1, F), zeros[1])
    assert pool.guided_result()[0].sum() == 0
    pool.guided_end()
    for call in (pool.guided_end, pool.gumbel_result, lambda: pool.gumbel_advance(*zeros),
                 lambda: raw("epa_gumbel_result", *out4)):
        with pytest.raises(ValueError, match="no guided-search session"):
            call()
    # a second begin with more roots than the first, after an end and without one
    pool.gumbel_begin(np.zeros((2, n_act), F), IDS[:2], 4, 2)
    pool.guided_end()
    pool.gumbel_begin(np.zeros((3, n_act), F), IDS[:3], 8, 2)
    _, _, results = pool_session(pool, IDS, 16, 16, np.zeros((N, n_act), F))
    assert (results[-1][0].sum(1) == np.where(ctx.st[IDS, 1] != 0, 0, 16)).all()
    pool.guided_end()
    assert np.array_equal(pool.get_state(), ctx.st)
    # the env classes: close() ends the session, and a pool can be closed with a session open
    env = envpool.make("TicTacToe-v1", "gymnasium", num_envs=8, seed=1)
    env.reset()
    gs = env.gumbel_search(simulations=4, seed=3)
    assert gs.leaves[2].tolist() == [0] * 8 and gs.leaves[1].all()
    gs.advance(*stand_in_logits(*gs.leaves[:2]))
    assert gs.result().visits.sum() == 0  # the first advance backs nothing up
    gs.advance(*stand_in_logits(*gs.leaves[:2]))
    assert (gs.result().visits.sum(1) == 1).all()
    gs.close()
    with pytest.raises(ValueError, match="closed"):
        gs.result()
    gs = env.gumbel_search([3, 1], simulations=4)
    gs.advance(*stand_in_logits(*gs.leaves[:2]))
    env.close()
    other = DevicePool("Othello", 4, seed=1)
    other.reset(np.arange(4, dtype=np.int32))
    other.recv_dict()
    other.gumbel_begin(np.zeros((4, 65), F), None, 8, 16)
    other.close()


def test_exact_values_give_minimax_optimal_moves_on_the_device(libs):
    """test_pgx_gumbel_host.py::test_exact_values_give_minimax_optimal_moves through the pool."""
    roots = two_ply_roots(Replayed(libs, "TicTacToe-v1", column=0))
    k = len(roots)
    pool = DevicePool("TicTacToe", k, seed=1)
    ids = np.arange(k, dtype=np.int32)
    pool.reset(ids)
    pool.recv_dict()
    pool.set_state(np.array([[2.0, 0.0] + p.key[1].tolist() for p in roots], np.float64), ids)
    memo = {}
    evaluate = exact_evaluator(memo)
    leaves = pool.gumbel_begin(np.zeros((k, 9), F), ids, 7, 16)
    for _ in range(8):
        leaves = pool.gumbel_advance(*evaluate(leaves[0], leaves[1]))
    visits, values, action, weights = pool.gumbel_result()
    pool.close()
    for i, pos in enumerate(roots):
        assert np.array_equal(visits[i], pos.mask.astype(np.int32))
        mine, theirs = tictactoe_cells(pos.obs)
        best = optimal_moves(mine, theirs, memo)
        assert int(action[i]) in best and int(np.argmax(weights[i])) in best
        for c in np.flatnonzero(pos.mask):
            assert values[i][c] == -minimax(theirs, mine | {int(c)}, memo)


def test_errors(libs):
    cart = DevicePool("CartPole", 4, seed=1)
    from envpool_amd.torch_interop import gumbel_search_device

    buf = np.zeros(64, np.float32)
    for call in (lambda: cart.gumbel_begin(np.zeros((4, 2), F)), lambda: gumbel_search_device(cart, None),
                 lambda: native.check(cart._lib.epa_gumbel_begin(cart._h, buf.ctypes.data, 2, 8, 2, 50.0, 0.1,
                                                                 buf.ctypes.data, buf.ctypes.data, buf.ctypes.data,
                                                                 buf.ctypes.data)),
                 lambda: native.check(cart._lib.epa_gumbel_result(cart._h, None, None, None, None))):
        with pytest.raises(RuntimeError, match="gumbel search not implemented"):
            call()
    cart.close()
    ctx = get_ctx(libs, "TicTacToe")
    pool = ctx.pool
    noise = np.zeros((N, 9), F)

    def raw_begin(simulations, considered, c_visit, c_scale, ids=IDS):
        ids = np.ascontiguousarray(ids, np.int32)
        obs, mask, status = np.zeros((N, 3, 3, 2), np.uint8), np.zeros((N, 9), np.uint8), np.zeros(N, np.uint8)
        native.check(pool._lib.epa_gumbel_begin(pool._h, ids.ctypes.data, len(ids), simulations, considered, c_visit,
                                                c_scale, noise.ctypes.data, obs.ctypes.data, mask.ctypes.data,
                                                status.ctypes.data))

    for args in ((0, 2, 50.0, 0.1), (4097, 2, 50.0, 0.1), (8, 0, 50.0, 0.1), (8, 2, -1.0, 0.1),
                 (8, 2, float("nan"), 0.1), (8, 2, 50.0, float("inf"))):
        with pytest.raises(ValueError, match="gumbel_begin"):
            raw_begin(*args)
    for ids in ([0, N], [-1]):
        with pytest.raises(ValueError):
            raw_begin(8, 2, 50.0, 0.1, ids=ids)
    with pytest.raises(ValueError, match="no guided-search session"):  # none of them opened one
        pool.guided_end()
    raw_begin(2, 1000, 50.0, 0.1)  # max_considered above the game's actions: all of them
    leaves = pool.gumbel_advance(*stand_in_logits(*pool.gumbel_begin(noise, IDS, 2, 1000)[:2]))
    good = stand_in_logits(leaves[0], leaves[1])
    for i, x in ((0, np.nan), (0, np.inf), (0, 2e30), (1, 2.0), (1, np.nan)):
        rows = [good[0].copy(), good[1].copy()]
        rows[i].reshape(-1)[3] = x
        with pytest.raises(ValueError, match="gumbel_advance"):
            pool.gumbel_advance(*rows)
        obs, mask, status = np.zeros((N, 3, 3, 2), np.uint8), np.zeros((N, 9), np.uint8), np.zeros(N, np.uint8)
        with pytest.raises(ValueError, match="gumbel_advance"):
            native.check(pool._lib.epa_gumbel_advance(pool._h, rows[0].ctypes.data, rows[1].ctypes.data, N,
                                                      obs.ctypes.data, mask.ctypes.data, status.ctypes.data))
    for _ in range(2):  # none of the refused calls counted: S + 1 = 3 advances pass, the fourth is above S
        leaves = pool.gumbel_advance(*stand_in_logits(leaves[0], leaves[1]))
    with pytest.raises(ValueError, match="above simulations"):
        pool.gumbel_advance(*good)
    pool.guided_end()
    assert np.array_equal(pool.get_state(), ctx.st) and np.array_equal(pool.snapshot(), ctx.S)


def teardown_module(module):
    for c in _ctx.values():
        c.pool.close()
    _ctx.clear()
