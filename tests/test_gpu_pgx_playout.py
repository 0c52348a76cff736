"""PGX playouts on the MI355X: the playout kernel against the pinned step path -- the same picks, made by the numpy
rule of pgx_playout_util.py from `info:legal_action_mask`, stepped ply by ply -- for all four games; the commit form
against the same plies stepped; independence of the launch shape; a sharded pool; the device form; the errors.

The shape: a pool of 70 envs (one full wave plus 6 lanes), a 37-long id subset in non-monotonic order, 3 repeats
(111 lanes), from positions a few plies into the game (TicTacToe: 6, so that some envs are over and some are not)."""
import ctypes

import numpy as np
import pytest

import envpool_amd as envpool
from envpool_amd.core import native
from envpool_amd.core.device_pool import DevicePool
from pgx_playout_util import pick, stream
from pgx_util import KEYS

pytestmark = pytest.mark.gpu

GAMES = ["TicTacToe", "ConnectFour", "Hex", "Othello"]
N, R, SEED, POOL_SEED = 70, 3, 15, 11
IDS = np.array([(i * 29 + 5) % N for i in range(37)], np.int32)  # distinct (29 and 70 are coprime), not monotonic
PRE = {"TicTacToe": 6, "ConnectFour": 3, "Hex": 3, "Othello": 3}
ALL = np.arange(N, dtype=np.int32)


def legal_random(mask, rng):
    mask = np.asarray(mask, bool)
    return (rng.random(mask.shape) * mask + mask).argmax(1).astype(np.int32)


def stepwise(pool, ctx, r, limit=256, ids=IDS):
    """restore(S), then the still-running listed envs stepped ply by ply with the picks of stream (id, r): what a
    playout of `limit` plies has to report.  Leaves the pool where those steps leave it."""
    pool.restore(ctx.S)
    k = len(ids)
    ret, plies = np.zeros((k, 2), np.float32), np.zeros(k, np.int32)
    running, mask = ~ctx.done0[ids], ctx.mask0[ids].copy()
    hs = [stream(SEED, int(i), r) for i in ids]
    for t in range(limit):
        idx = np.flatnonzero(running)
        if len(idx) == 0:
            break
        act = np.array([pick(mask[j], hs[j], t) for j in idx], np.int32)
        pool.send(ids[idx], act)
        out = pool.recv_dict()
        assert np.array_equal(out["info:env_id"], ids[idx])
        ret[idx] += np.asarray(out["reward"]).reshape(len(idx), 2)
        plies[idx] += 1
        mask[idx] = out["info:legal_action_mask"]
        running[idx] = ~np.asarray(out["done"], bool)
    return ret, plies, running.astype(np.uint8)


class Ctx:
    """One pool per game, a few plies in, with its snapshot S; the stepwise expectations are computed once."""

    def __init__(self, fam):
        self.fam = fam
        self.pool = pool = DevicePool(fam, N, seed=POOL_SEED)
        pool.reset(ALL)
        out = pool.recv_dict()
        rng = np.random.default_rng(2)
        for _ in range(PRE[fam]):
            pool.send(ALL, legal_random(out["info:legal_action_mask"], rng))
            out = pool.recv_dict()
        assert np.array_equal(out["info:env_id"], ALL)
        self.mask0 = np.asarray(out["info:legal_action_mask"], bool).copy()
        self.done0 = np.asarray(out["done"], bool).copy()
        self.S = pool.snapshot()
        self.st = pool.get_state()
        self._want = None
        self._twin = None

    def want(self):
        """(returns [k, R, 2], plies [k, R], status [k, R]) of whole games by the step path."""
        if self._want is None:
            per_r = [stepwise(self.pool, self, r) for r in range(R)]
            self._want = tuple(np.stack([x[i] for x in per_r], axis=1) for i in range(3))
        return self._want

    def twin(self):
        """The commit test's other side: four stepwise plies of repeat 0, then one step of every listed env."""
        if self._twin is None:
            res = stepwise(self.pool, self, 0, limit=4)
            st, snap = self.pool.get_state(), self.pool.snapshot(rng=True)
            self.pool.send(IDS, np.zeros(len(IDS), np.int32))
            rows = {k: np.asarray(v).copy() for k, v in self.pool.recv_dict().items()}
            self._twin = (res, st, snap, rows)
        return self._twin


_ctx = {}


@pytest.fixture(scope="module", params=GAMES)
def ctx(request):
    fam = request.param
    if fam not in _ctx:
        _ctx[fam] = Ctx(fam)
    return _ctx[fam]


def test_setup_positions(ctx):
    done = ctx.done0[IDS]
    if ctx.fam == "TicTacToe":
        assert done.any() and not done.all()
    assert len(np.unique(ctx.st[:, 2:], axis=0)) > N // 2  # the positions differ


def test_playout_agrees_with_the_step_path_and_changes_nothing(ctx):
    pool = ctx.pool
    pool.restore(ctx.S)
    returns, plies, status = pool.playout(IDS, repeats=R, seed=SEED)
    assert returns.shape == (len(IDS), R, 2) and returns.dtype == np.float32
    assert plies.shape == (len(IDS), R) and plies.dtype == np.int32
    assert status.shape == (len(IDS), R) and status.dtype == np.uint8
    assert np.array_equal(pool.get_state(), ctx.st)
    assert np.array_equal(pool.snapshot(), ctx.S)
    want = ctx.want()
    assert np.array_equal(plies, want[1]), ctx.fam
    assert np.array_equal(returns, want[0]), ctx.fam
    assert np.array_equal(status, want[2]) and (status == 0).all(), ctx.fam
    assert (plies[ctx.done0[IDS]] == 0).all() and (plies[~ctx.done0[IDS]] > 0).all()


def test_commit_equals_the_plies_stepped(ctx):
    pool = ctx.pool
    (w_ret, w_plies, w_status), w_st, w_snap, w_rows = ctx.twin()
    pool.restore(ctx.S)
    returns, plies, status = pool.playout(IDS, max_plies=4, seed=SEED, commit=True)
    assert np.array_equal(returns[:, 0], w_ret) and np.array_equal(plies[:, 0], w_plies)
    assert np.array_equal(status[:, 0], w_status)
    assert np.array_equal(pool.get_state(), w_st)
    assert np.array_equal(pool.snapshot(rng=True), w_snap)
    pool.send(IDS, np.zeros(len(IDS), np.int32))
    rows = pool.recv_dict()
    for k in KEYS:
        assert np.array_equal(np.asarray(rows[k]), w_rows[k]), (ctx.fam, k)
    ended = ctx.done0[IDS] | ((status[:, 0] == 0) & (plies[:, 0] > 0))
    assert np.array_equal(np.asarray(rows["elapsed_step"]) == 0, ended)  # the next step resets exactly those
    if ctx.fam != "TicTacToe":
        assert (status == 1).any()


def test_launch_shape_independence(ctx):
    pool = ctx.pool
    pool.restore(ctx.S)
    want = ctx.want()
    rev = pool.playout(IDS[::-1].copy(), repeats=R, seed=SEED)
    one = pool.playout(IDS, repeats=1, seed=SEED)
    for got_rev, got_one, w in zip(rev, one, want):
        assert np.array_equal(got_rev, w[::-1])
        assert np.array_equal(got_one[:, 0], w[:, 0])
    whole = pool.playout(None, repeats=2, seed=SEED)  # the whole pool: the identity id table
    for got, w in zip(whole, want):
        assert np.array_equal(got[IDS], w[:, :2])
    other = pool.playout(IDS, repeats=R, seed=SEED + 1)
    assert not np.array_equal(other[1], want[1]) or ctx.fam == "TicTacToe"


@pytest.mark.parametrize("fam", GAMES)
def test_sharded_pool_equals_the_unsharded(fam):
    """device=[0, 0]: two shards, the second with env_id_offset 35; the streams are keyed by the global id."""
    results = []
    for device in ([0, 0], 0):
        env = envpool.make(f"{fam}-v1", "gymnasium", num_envs=N, device=device, seed=POOL_SEED)
        _, info = env.reset()
        rng = np.random.default_rng(2)
        for _ in range(PRE[fam]):
            _, _, _, _, info = env.step(legal_random(info["legal_action_mask"], rng))
        out = env.playout(IDS, repeats=R, seed=SEED)
        assert out._fields == ("returns", "plies", "status")
        results.append(out)
        env.close()
    assert (IDS < N // 2).any() and (IDS >= N // 2).any() and (np.diff(IDS // (N // 2)) != 0).sum() > 2
    for a, b in zip(*results):
        assert np.array_equal(a, b)
    assert results[0].plies.max() > 0


def test_device_form(ctx):
    import torch

    from envpool_amd.torch_interop import playout_device, recv_device_tensors, send_device_tensors

    pool = ctx.pool
    want = ctx.want()
    (w_ret, w_plies, w_status), _, _, w_rows = ctx.twin()
    pool.restore(ctx.S)
    got = playout_device(pool, IDS, repeats=R, seed=SEED)
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32 and got[2].dtype == torch.uint8
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), w)
    # a step enqueued right behind a committing playout sees the committed state
    pool.restore(ctx.S)
    ids_t = torch.as_tensor(IDS, device="cuda:0")
    act = torch.zeros(len(IDS), dtype=torch.int32, device="cuda:0")
    ret, plies, status = playout_device(pool, IDS, max_plies=4, seed=SEED, commit=True)
    send_device_tensors(pool, act, ids_t)
    rows = {k: v.cpu().numpy() for k, v in recv_device_tensors(pool).items()}
    assert np.array_equal(ret.cpu().numpy()[:, 0], w_ret) and np.array_equal(plies.cpu().numpy()[:, 0], w_plies)
    assert np.array_equal(status.cpu().numpy()[:, 0], w_status)
    for k in KEYS:
        assert np.array_equal(rows[k].reshape(w_rows[k].shape), w_rows[k]), (ctx.fam, k)


def _raw(pool, ids, repeats, max_plies, flags):
    """epa_playout itself, past the wrapper's checks."""
    ids = np.ascontiguousarray(ids, np.int32)
    t = max(len(ids) * max(repeats, 1), 1)
    ret, plies, status = np.zeros((t, 2), np.float32), np.zeros(t, np.int32), np.zeros(t, np.uint8)
    native.check(pool._lib.epa_playout(pool._h, ids.ctypes.data, len(ids), repeats, max_plies, ctypes.c_uint64(SEED),
                                       flags, ret.ctypes.data, plies.ctypes.data, status.ctypes.data))


def test_errors():
    cart = DevicePool("CartPole", 4, seed=1)
    with pytest.raises(RuntimeError, match="playout not implemented"):
        cart.playout(None)
    from envpool_amd.torch_interop import playout_device

    with pytest.raises(RuntimeError, match="playout not implemented"):
        playout_device(cart, None)
    cart.close()
    if "TicTacToe" not in _ctx:
        _ctx["TicTacToe"] = Ctx("TicTacToe")
    ctx = _ctx["TicTacToe"]
    pool = ctx.pool
    pool.restore(ctx.S)
    for kw in (dict(repeats=0), dict(repeats=4097), dict(max_plies=-1), dict(max_plies=257),
               dict(repeats=2, commit=True)):
        with pytest.raises(ValueError, match="playout"):
            pool.playout(IDS, **kw)
    for bad in ([0, N], [-1], [0, 1, 0]):
        with pytest.raises(ValueError):
            pool.playout(np.array(bad, np.int32), commit=True)
    with pytest.raises(ValueError, match="exceeds num_envs"):
        pool.playout(np.zeros(N + 1, np.int32))
    # the engine's own checks, behind the wrapper's
    for args in ((IDS, 0, 0, 0), (IDS, 4097, 0, 0), (IDS, 1, -1, 0), (IDS, 1, 257, 0), (IDS, 1, 0, 2),
                 (IDS, 2, 0, native.EPA_PLAYOUT_COMMIT), ([3, 4, 3], 1, 0, native.EPA_PLAYOUT_COMMIT),
                 ([N], 1, 0, 0), (IDS[:0], 1, 0, 0)):
        with pytest.raises(ValueError):
            _raw(pool, *args)
    # nothing was touched, and the pool plays and steps as before
    assert np.array_equal(pool.get_state(), ctx.st) and np.array_equal(pool.snapshot(), ctx.S)
    got = pool.playout(IDS, repeats=1, seed=SEED)
    ret, plies, status = stepwise(pool, ctx, 0)
    assert np.array_equal(got[0][:, 0], ret) and np.array_equal(got[1][:, 0], plies)
    assert np.array_equal(got[2][:, 0], status)


def teardown_module(module):
    for c in _ctx.values():
        c.pool.close()
    _ctx.clear()
