"""PGX tree search on the MI355X: the search kernel against the host harness of the same header fed the pool's own
hidden words, for all four games; against the contract rebuilt from public calls only (restore, send / recv, snapshot,
playout) with numpy scores; independence of id order and sharding; the device form; the errors.

The shape: a pool of 70 envs a few plies into their games with one env marked over, 11 ids out of order (11 blocks of
one wave), S = 24 simulations of R = 4 leaf playouts (Hex: S = 12)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import envpool_amd as envpool
from envpool_amd.core import native
from envpool_amd.core.device_pool import DevicePool
from pgx_search_util import Pos, puct_search
from pgx_util import ACTIONS, CODE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMES = ["TicTacToe", "ConnectFour", "Hex", "Othello"]
N, R, SEED, POOL_SEED, C_PUCT = 70, 4, 15, 11, 1.25
SIMS = {"TicTacToe": 24, "ConnectFour": 24, "Hex": 12, "Othello": 24}
PRE = {"TicTacToe": 4, "ConnectFour": 3, "Hex": 3, "Othello": 3}
OVER = 33  # the env marked over
IDS = np.array([41, 7, 69, OVER, 0, 64, 12, 63, 5, 50, 22], np.int32)  # 11 ids, not monotonic, both sides of lane 64
ALL = np.arange(N, dtype=np.int32)


def legal_random(mask, rng):
    mask = np.asarray(mask, bool)
    return (rng.random(mask.shape) * mask + mask).argmax(1).astype(np.int32)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pgx_search") / "libpgxsearchhost.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "cpu_harness", "pgx_search_host.cpp"), "-o", out], check=True)
    return ctypes.CDLL(out)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_search(lib, fam, st, ids, simulations, leaf_playouts, c_puct, max_plies, seed):
    """The harness on rows of get_state ([cur_step, done, hidden words]) with the global ids `ids`."""
    n_act, k = ACTIONS[fam], len(ids)
    hid = np.ascontiguousarray(st[:, 2:], np.int32)
    done = np.ascontiguousarray(st[:, 1] != 0, np.uint8)
    visits, returns = np.full((k, n_act), -7, np.int32), np.full((k, n_act), -7, np.int32)
    action, nodes = np.full(k, -7, np.int32), np.zeros(k, np.int32)
    rc = lib.pgx_search(CODE[fam], k, _ptr(hid), _ptr(done), _ptr(np.ascontiguousarray(ids, np.int32)), simulations,
                        leaf_playouts, ctypes.c_float(c_puct), max_plies, ctypes.c_uint64(seed), _ptr(visits),
                        _ptr(returns), _ptr(action), _ptr(nodes))
    assert rc == 0
    return visits, returns, action


def rolled(fam, step):
    """PRE[fam] seeded random legal plies of every env through `step(actions) -> legal mask`."""
    rng = np.random.default_rng(2)
    mask = step(None)
    for _ in range(PRE[fam]):
        mask = step(legal_random(mask, rng))
    return mask


class Ctx:
    """One pool per game, a few plies in, env OVER marked over, with its state, snapshot and one search."""

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
            self.mover0 = np.asarray(out["info:current_player"]).copy()
            return out["info:legal_action_mask"]

        self.mask0 = np.asarray(rolled(fam, step), bool).copy()
        row = pool.get_state([OVER])
        row[0, 1] = 1.0
        pool.set_state(row, [OVER])
        self.st = pool.get_state()
        self.S = pool.snapshot()
        self.got = pool.search(IDS, SIMS[fam], R, C_PUCT, 0, SEED)


_ctx = {}


@pytest.fixture(scope="module", params=GAMES)
def ctx(request):
    fam = request.param
    if fam not in _ctx:
        _ctx[fam] = Ctx(fam)
    return _ctx[fam]


def test_kernel_equals_the_host_harness_and_changes_nothing(ctx, harness):
    fam, n_act = ctx.fam, ACTIONS[ctx.fam]
    visits, returns, action = ctx.got
    assert visits.shape == (len(IDS), n_act) and visits.dtype == np.int32
    assert returns.shape == (len(IDS), n_act) and returns.dtype == np.int32
    assert action.shape == (len(IDS),) and action.dtype == np.int32
    assert np.array_equal(ctx.pool.get_state(), ctx.st)
    assert np.array_equal(ctx.pool.snapshot(), ctx.S)
    over = ctx.st[IDS, 1] != 0
    assert over[list(IDS).index(OVER)] and not over.all()
    assert len(np.unique(ctx.st[IDS][:, 2:], axis=0)) > len(IDS) // 2  # the positions differ
    want = host_search(harness, fam, ctx.st[IDS], IDS, SIMS[fam], R, C_PUCT, 0, SEED)
    assert np.array_equal(visits, want[0]), fam
    assert np.array_equal(returns, want[1]), fam
    assert np.array_equal(action, want[2]), fam
    assert (action[over] == -1).all() and not visits[over].any() and not returns[over].any()
    assert (visits[~over].sum(1) == SIMS[fam]).all() and (action[~over] >= 0).all()
    # another seed, c_puct and a cut of the playouts: still the harness
    got = ctx.pool.search(IDS[:5], SIMS[fam], 3, 0.0, 6, SEED + 1)
    want = host_search(harness, fam, ctx.st[IDS[:5]], IDS[:5], SIMS[fam], 3, 0.0, 6, SEED + 1)
    for g, w in zip(got, want):
        assert np.array_equal(g, w), fam


@pytest.mark.parametrize("fam", ["TicTacToe", "Othello"])
def test_search_rebuilt_from_public_calls(fam):
    """The tree in Python; a node is a single-env snapshot; expansion is restore + send / recv + snapshot in env e,
    a leaf value the last R of playout([e], repeats=(t + 1) * R); scores in numpy (pgx_search_util.py)."""
    if fam not in _ctx:
        _ctx[fam] = Ctx(fam)
    ctx = _ctx[fam]
    pool = ctx.pool
    sims, roots = 16, [i for i in IDS if i != OVER][:4]
    got = pool.search(np.array(roots, np.int32), sims, R, C_PUCT, 0, SEED)
    for j, e in enumerate(roots):
        ids = np.array([e], np.int32)

        def expand(pos, a):
            pool.restore(pos.key, ids)
            pool.send(ids, np.array([a], np.int32))
            out = pool.recv_dict()
            rw = np.asarray(out["reward"]).reshape(2)
            assert rw[0] == -rw[1]
            new = Pos(mask=np.asarray(out["info:legal_action_mask"], bool).reshape(-1), done=bool(out["done"][0]),
                      mover=int(out["info:current_player"][0]), key=pool.snapshot(ids))
            return new, int(rw[0])

        def leaf(pos, t):
            pool.restore(pos.key, ids)
            ret = pool.playout(ids, repeats=(t + 1) * R, seed=SEED)[0][0, -R:]
            assert np.array_equal(ret[:, 0], -ret[:, 1])
            return int(ret[:, 0].sum())

        pool.restore(ctx.S)
        root = Pos(mask=ctx.mask0[e], done=False, mover=int(ctx.mover0[e]), key=pool.snapshot(ids))
        want = puct_search(root, expand, leaf, sims, R, C_PUCT)
        pool.restore(ctx.S)
        assert np.array_equal(got[0][j], want[0]), (fam, e)
        assert np.array_equal(got[1][j], want[1]), (fam, e)
        assert got[2][j] == want[2], (fam, e)
    assert np.array_equal(pool.get_state(), ctx.st)


def test_id_order_and_device_form(ctx):
    import torch

    from envpool_amd.torch_interop import search_device

    pool, fam = ctx.pool, ctx.fam
    perm = np.random.default_rng(4).permutation(len(IDS))
    got = pool.search(IDS[perm], SIMS[fam], R, C_PUCT, 0, SEED)
    for g, w in zip(got, ctx.got):
        assert np.array_equal(g, w[perm])
    twice = pool.search(np.array([IDS[1], IDS[1], IDS[0]], np.int32), SIMS[fam], R, C_PUCT, 0, SEED)  # ids may repeat
    for g, w in zip(twice, ctx.got):
        assert np.array_equal(g, w[[1, 1, 0]])
    whole = pool.search(None, 4, 2, C_PUCT, 0, SEED)  # the whole pool: the identity id table, 70 blocks
    part = pool.search(IDS, 4, 2, C_PUCT, 0, SEED)
    for g, w in zip(whole, part):
        assert np.array_equal(g[IDS], w)
    dev = search_device(pool, IDS, SIMS[fam], R, C_PUCT, 0, SEED)
    assert all(t.dtype == torch.int32 and t.is_cuda for t in dev)
    for g, w in zip(dev, ctx.got):
        assert np.array_equal(g.cpu().numpy(), w)
    other = pool.search(IDS, SIMS[fam], R, C_PUCT, 0, SEED + 1)
    assert not np.array_equal(other[1], ctx.got[1])
    assert np.array_equal(pool.get_state(), ctx.st) and np.array_equal(pool.snapshot(), ctx.S)


@pytest.mark.parametrize("fam", GAMES)
def test_sharded_pool_equals_the_unsharded(fam):
    """device=[0, 0]: two shards, the second with env_id_offset 35; the leaf playouts are keyed by the global id."""
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
        out = env.search(IDS, simulations=SIMS[fam], leaf_playouts=R, c_puct=C_PUCT, seed=SEED)
        assert out._fields == ("visits", "returns", "action")
        results.append(out)
        env.close()
    assert (IDS < N // 2).any() and (IDS >= N // 2).any() and (np.diff(IDS // (N // 2)) != 0).sum() > 2
    for a, b in zip(*results):
        assert np.array_equal(a, b)
    assert results[0].visits.sum() > 0


def _raw(pool, ids, simulations, leaf_playouts, c_puct, max_plies, n_act):
    """epa_search itself, past the wrapper's checks."""
    ids = np.ascontiguousarray(ids, np.int32)
    k = max(len(ids), 1)
    visits, returns, action = np.zeros((k, n_act), np.int32), np.zeros((k, n_act), np.int32), np.zeros(k, np.int32)
    native.check(pool._lib.epa_search(pool._h, ids.ctypes.data, len(ids), simulations, leaf_playouts,
                                      ctypes.c_float(c_puct), max_plies, ctypes.c_uint64(SEED), visits.ctypes.data,
                                      returns.ctypes.data, action.ctypes.data))
    return visits, returns, action


def test_errors():
    cart = DevicePool("CartPole", 4, seed=1)
    with pytest.raises(RuntimeError, match="search not implemented"):
        cart.search(None)
    from envpool_amd.torch_interop import search_device

    with pytest.raises(RuntimeError, match="search not implemented"):
        search_device(cart, None)
    cart.close()
    if "TicTacToe" not in _ctx:
        _ctx["TicTacToe"] = Ctx("TicTacToe")
    ctx = _ctx["TicTacToe"]
    pool = ctx.pool
    bad = [dict(simulations=0), dict(simulations=4097), dict(leaf_playouts=0), dict(leaf_playouts=65),
           dict(simulations=1025, leaf_playouts=4), dict(max_plies=-1), dict(max_plies=257), dict(c_puct=-1.0),
           dict(c_puct=float("nan")), dict(c_puct=float("inf"))]
    base = dict(simulations=8, leaf_playouts=2, c_puct=C_PUCT, max_plies=0)
    for kw in bad:
        with pytest.raises(ValueError, match="search"):
            pool.search(IDS, **{**base, **kw})
        a = {**base, **kw}
        with pytest.raises(ValueError, match="search"):
            _raw(pool, IDS, a["simulations"], a["leaf_playouts"], a["c_puct"], a["max_plies"], 9)
    # the id checks of snapshot, through both
    for ids in ([0, N], [-1], []):
        with pytest.raises(ValueError):
            pool.search(np.array(ids, np.int32), **base)
        with pytest.raises(ValueError):
            _raw(pool, ids, 8, 2, C_PUCT, 0, 9)
    with pytest.raises(ValueError, match="exceeds num_envs"):
        pool.search(np.zeros(N + 1, np.int32), **base)
    with pytest.raises(ValueError, match="exceeds num_envs"):
        _raw(pool, np.zeros(N + 1, np.int32), 8, 2, C_PUCT, 0, 9)
    # nothing was touched, and the pool searches as before
    assert np.array_equal(pool.get_state(), ctx.st) and np.array_equal(pool.snapshot(), ctx.S)
    again = _raw(pool, IDS, SIMS["TicTacToe"], R, C_PUCT, 0, 9)
    for g, w in zip(again, ctx.got):
        assert np.array_equal(g, w)


def test_tree_scratch_above_2_gib_is_refused(harness):
    """Hex with 4096 simulations: 4097 nodes per root; the message names the most roots that fit."""
    node = harness.pgx_search_node_bytes(CODE["Hex"])
    fits = 2**31 // (4097 * node)
    pool = DevicePool("Hex", fits + 8, seed=1)
    pool.reset(np.arange(fits + 8, dtype=np.int32))
    pool.recv_dict()
    st = pool.get_state()
    with pytest.raises(ValueError, match=f"at most {fits} roots"):
        pool.search(np.arange(fits + 1, dtype=np.int32), 4096, 1, C_PUCT, 0, SEED)
    with pytest.raises(ValueError, match=f"at most {fits} roots"):
        _raw(pool, np.arange(fits + 1, dtype=np.int32), 4096, 1, C_PUCT, 0, 122)
    assert np.array_equal(pool.get_state(), st)
    out = pool.search(np.arange(3, dtype=np.int32), 8, 1, C_PUCT, 0, SEED)  # and the pool still searches
    assert (out[0].sum(1) == 8).all()
    pool.close()


def teardown_module(module):
    for c in _ctx.values():
        c.pool.close()
    _ctx.clear()
