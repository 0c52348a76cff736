"""PGX exact solver on the MI355X: the solve kernel against the host harness of the same header fed the pool's own
hidden words (all five outputs) and against the brute-force minimax that shares nothing with either (value, q, action,
status), for all four games at the horizons of the host test; hand-made positions put in with set_state; late Othello to
the end of the game; that nothing of the pool changes; independence of id order, repeated ids and sharding; the device
form; the errors.

The shape: a pool of 70 envs a few plies into their games with one env marked over and two holding the hand-made
positions, 11 ids out of order on both sides of lane 64 (11 blocks of one wave)."""
import ctypes

import numpy as np
import pytest

import envpool_amd as envpool
from envpool_amd.core import native
from envpool_amd.core.device_pool import DevicePool
from pgx_solve_util import BIG, DEPTHS, GAMES, LATE_PLIES, brute_solve, build, hand_made, host_solve, rolled
from pgx_util import ACTIONS

pytestmark = pytest.mark.gpu

N, SEED, POOL_SEED = 70, 15, 11
PRE = {"TicTacToe": 2, "ConnectFour": 3, "Hex": 3, "Othello": 3}
OVER = 33  # the env marked over
WIN, LOSS = 7, 64  # the envs that hold the hand-made positions
IDS = np.array([41, WIN, 69, OVER, 0, LOSS, 12, 63, 5, 50, 22], np.int32)  # not monotonic, both sides of lane 64
ALL = np.arange(N, dtype=np.int32)
NAMES = ("value", "q", "action", "status", "nodes")


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pgx_solve")
    return {s: build(tmp, f"pgx_{s}.cpp") for s in ("solve_host", "solve_brute")}


def same(got, want, what, names=NAMES):
    for name, g, w in zip(names, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        assert np.array_equal(g, w), (what, name, np.flatnonzero((g != w).reshape(len(g), -1).any(1)))


def check(libs, fam, st, got, depth, max_nodes=BIG):
    """`got` of rows `st` of get_state ([cur_step, done, hidden words]): the harness in all five outputs, the brute
    force in the first four (every row solved or over)."""
    hid, done = st[:, 2:].astype(np.int32), (st[:, 1] != 0).astype(np.uint8)
    want, broken = host_solve(libs["solve_host"], fam, hid, done, depth, max_nodes)
    assert not broken.any()
    same(got, want, (fam, depth, "harness"))
    if max_nodes == BIG:
        same(got[:4], brute_solve(libs["solve_brute"], fam, hid, done, depth)[0], (fam, depth, "brute force"))
    return want


class Ctx:
    """One pool per game, a few plies in, env OVER marked over, envs WIN and LOSS at the hand-made positions, with its
    state, snapshot and the solves at the game's horizons."""

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
            return out["info:legal_action_mask"]

        rolled(step, PRE[fam])
        rows = pool.get_state([OVER, WIN, LOSS])
        rows[0, 1] = 1.0
        self.hand = hand_made(fam)
        rows[1, 2:], rows[2, 2:] = self.hand[0][0], self.hand[1][0]
        pool.set_state(rows, [OVER, WIN, LOSS])
        self.st = pool.get_state()
        self.S = pool.snapshot()
        self.got = {d: pool.solve(IDS, d, BIG) for d in DEPTHS[fam] + [3, 2]}


_ctx = {}


@pytest.fixture(scope="module", params=GAMES)
def ctx(request):
    fam = request.param
    if fam not in _ctx:
        _ctx[fam] = Ctx(fam)
    return _ctx[fam]


def test_kernel_equals_the_harness_and_the_brute_force(ctx, libs):
    fam, n_act = ctx.fam, ACTIONS[ctx.fam]
    over = ctx.st[IDS, 1] != 0
    assert over[list(IDS).index(OVER)] and over.sum() == 1
    assert len(np.unique(ctx.st[IDS][:, 2:], axis=0)) > len(IDS) // 2  # the positions differ
    for depth in DEPTHS[fam]:
        value, q, action, status, nodes = ctx.got[depth]
        assert q.shape == (len(IDS), n_act) and q.dtype == np.int8 and value.dtype == np.int8
        assert action.dtype == np.int32 and status.dtype == np.uint8 and nodes.dtype == np.int64
        check(libs, fam, ctx.st[IDS], ctx.got[depth], depth)
        assert np.array_equal(status, np.where(over, 2, 0))
        assert (value[over] == 0).all() and (action[over] == -1).all() and (q[over] == -128).all()
        legal = q[~over] != -128
        assert (legal.sum(1) > 1).all() and (q[~over].max(1) == value[~over]).all() and (nodes[~over] > 1).all()
    # the hand-made positions: a forced win in 3 plies and not in 2, a forced loss in 2 plies
    w, l = list(IDS).index(WIN), list(IDS).index(LOSS)
    for depth in (3, 2):
        check(libs, fam, ctx.st[IDS], ctx.got[depth], depth)
    assert [ctx.hand[0][1], ctx.hand[1][1]] == [3, 2]
    assert ctx.got[3][0][w] == 1 and ctx.got[2][0][w] == 0 and ctx.got[2][0][l] == -1 and ctx.got[3][0][l] == -1
    assert ctx.got[3][1][w, ctx.got[3][2][w]] == 1


def test_nothing_of_the_pool_changes(ctx):
    pool = ctx.pool
    pool.solve(IDS, DEPTHS[ctx.fam][0], BIG)
    assert np.array_equal(pool.get_state(), ctx.st)
    assert np.array_equal(pool.snapshot(), ctx.S)
    # the next recv: the same step after a solve and after none
    outs = []
    for solve_first in (True, False):
        pool.restore(ctx.S)
        if solve_first:
            pool.solve(None, 2, BIG)
        pool.send(ALL, np.zeros(N, np.int32))
        outs.append(pool.recv_dict())
    assert sorted(outs[0]) == sorted(outs[1])
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k
    pool.restore(ctx.S)
    assert np.array_equal(pool.get_state(), ctx.st)


def test_id_order_repeats_and_device_form(ctx):
    import torch

    from envpool_amd.torch_interop import solve_device

    pool, depth = ctx.pool, DEPTHS[ctx.fam][-1]
    first = ctx.got[depth]
    same(pool.solve(IDS, depth, BIG), first, "the same call twice")
    perm = np.random.default_rng(4).permutation(len(IDS))
    same(pool.solve(IDS[perm], depth, BIG), [w[perm] for w in first], "id order")
    same(pool.solve(np.array([IDS[1], IDS[1], IDS[0]], np.int32), depth, BIG), [w[[1, 1, 0]] for w in first], "repeats")
    whole = pool.solve(None, depth, BIG)  # the whole pool: the identity id table, 70 blocks
    same([g[IDS] for g in whole], first, "whole pool")
    dev = solve_device(pool, IDS, depth, BIG)
    assert all(t.is_cuda for t in dev)
    assert [t.dtype for t in dev] == [torch.int8, torch.int8, torch.int32, torch.uint8, torch.int64]
    same([t.cpu().numpy() for t in dev], first, "device form")
    assert np.array_equal(pool.get_state(), ctx.st) and np.array_equal(pool.snapshot(), ctx.S)


@pytest.fixture(scope="module")
def late():
    """Othello LATE_PLIES plies in by committed playouts, env OVER marked over."""
    pool = DevicePool("Othello", N, seed=POOL_SEED)
    pool.reset(ALL)
    pool.recv_dict()
    pool.playout(ALL, 1, LATE_PLIES, SEED, commit=True)
    row = pool.get_state([OVER])
    row[0, 1] = 1.0
    pool.set_state(row, [OVER])
    yield pool, pool.get_state()
    pool.close()


def test_late_othello_to_the_end_of_the_game(late, libs):
    pool, st = late
    got = pool.solve(IDS, 0, BIG)
    check(libs, "Othello", st[IDS], got, 0)
    run = got[3] == 0
    assert run.sum() == len(IDS) - 1 and set(np.unique(got[0][run])) <= {-1, 0, 1} and len(np.unique(got[0][run])) > 1
    same(pool.solve(IDS, 0, BIG), got, "the same call twice")
    # max_nodes = 1: at least two plies are left, so every running root is given up
    value, q, action, status, nodes = pool.solve(IDS, 0, 1)
    assert np.array_equal(status, np.where(run, 1, 2))
    assert (value == 0).all() and (action == -1).all() and (q == -128).all() and (nodes[run] > 1).all()
    # a budget between the trees' sizes: the rows the harness gives up, and its `nodes`
    budget = int(np.median(got[4][run]))
    tight = pool.solve(IDS, 0, budget)
    check(libs, "Othello", st[IDS], tight, 0, budget)
    assert (tight[3] == 1).any() and (tight[3] == 0).any()
    assert np.array_equal(pool.get_state(), st)


@pytest.mark.parametrize("fam", GAMES)
def test_sharded_pool_equals_the_unsharded(fam):
    """device=[0, 0]: two shards, the second with env_id_offset 35."""
    results = []
    for device in ([0, 0], 0):
        env = envpool.make(f"{fam}-v1", "gymnasium", num_envs=N, device=device, seed=POOL_SEED)

        def step(act):
            if act is None:
                _, info = env.reset()
            else:
                _, _, _, _, info = env.step(act)
            return info["legal_action_mask"]

        rolled(step, PRE[fam])
        out = env.solve(IDS, depth=DEPTHS[fam][0], max_nodes=BIG)
        assert out._fields == NAMES
        results.append(out)
        env.close()
    assert (IDS < N // 2).any() and (IDS >= N // 2).any() and (np.diff(IDS // (N // 2)) != 0).sum() > 2
    same(results[0], results[1], (fam, "sharded"))
    assert (results[0].status == 0).all() and (results[0].nodes > 1).all()


def _raw(pool, ids, depth, max_nodes, n_act):
    """epa_solve itself, past the wrapper's checks."""
    ids = np.ascontiguousarray(ids, np.int32)
    k = max(len(ids), 1)
    value, q, action = np.zeros(k, np.int8), np.zeros((k, n_act), np.int8), np.zeros(k, np.int32)
    status, nodes = np.zeros(k, np.uint8), np.zeros(k, np.int64)
    native.check(pool._lib.epa_solve(pool._h, ids.ctypes.data, len(ids), depth, ctypes.c_int64(max_nodes),
                                     value.ctypes.data, q.ctypes.data, action.ctypes.data, status.ctypes.data,
                                     nodes.ctypes.data))
    return value, q, action, status, nodes


def test_errors():
    from envpool_amd.torch_interop import solve_device

    cart = DevicePool("CartPole", 4, seed=1)
    with pytest.raises(RuntimeError, match="solve not implemented for this environment"):
        cart.solve(None)
    with pytest.raises(RuntimeError, match="solve not implemented for this environment"):
        solve_device(cart, None)
    with pytest.raises(RuntimeError, match="solve not implemented for this environment"):
        _raw(cart, [0], 0, 1, 9)
    cart.close()
    env = envpool.make("CartPole-v1", "gymnasium", num_envs=4, seed=1)
    with pytest.raises(RuntimeError, match="solve not implemented for this environment"):
        env.solve()
    env.close()
    if "TicTacToe" not in _ctx:
        _ctx["TicTacToe"] = Ctx("TicTacToe")
    ctx = _ctx["TicTacToe"]
    pool = ctx.pool
    for kw, text in ((dict(depth=-1), "depth = -1 must be 0 .. 128"), (dict(depth=129), "depth = 129 must be 0 .. 128"),
                     (dict(max_nodes=0), "max_nodes = 0 must be at least 1"),
                     (dict(max_nodes=-5), "max_nodes = -5 must be at least 1")):
        a = {**dict(depth=0, max_nodes=1 << 20), **kw}
        with pytest.raises(ValueError, match="solve: " + text):
            pool.solve(IDS, **a)
        with pytest.raises(ValueError, match="solve: " + text):
            _raw(pool, IDS, a["depth"], a["max_nodes"], 9)
    # the id checks of search, through both
    for ids in ([0, N], [-1], []):
        with pytest.raises(ValueError):
            pool.solve(np.array(ids, np.int32))
        with pytest.raises(ValueError):
            _raw(pool, ids, 0, 1 << 20, 9)
    with pytest.raises(ValueError, match="exceeds num_envs"):
        pool.solve(np.zeros(N + 1, np.int32))
    with pytest.raises(ValueError, match="exceeds num_envs"):
        _raw(pool, np.zeros(N + 1, np.int32), 0, 1 << 20, 9)
    # nothing was touched, and the pool solves as before
    assert np.array_equal(pool.get_state(), ctx.st) and np.array_equal(pool.snapshot(), ctx.S)
    same(_raw(pool, IDS, 0, BIG, 9), ctx.got[0], "after the refusals")


def test_stacks_above_2_gib_are_refused(libs):
    """D = 0: 128 plies x 64 lanes x 80 bytes per root; the message names the most roots that fit."""
    libs["solve_host"].pgx_solve_stack_bytes.restype = ctypes.c_longlong
    per_root = libs["solve_host"].pgx_solve_stack_bytes(0)
    fits = 2**31 // per_root
    assert per_root == 128 * 64 * 80 and fits == 3276
    pool = DevicePool("TicTacToe", fits + 8, seed=1)
    pool.reset(np.arange(fits + 8, dtype=np.int32))
    pool.recv_dict()
    st = pool.get_state()
    with pytest.raises(ValueError, match=f"at most {fits} roots"):
        pool.solve(np.arange(fits + 1, dtype=np.int32), 0)
    with pytest.raises(ValueError, match=f"at most {fits} roots"):
        _raw(pool, np.arange(fits + 1, dtype=np.int32), 0, 1 << 20, 9)
    assert np.array_equal(pool.get_state(), st)
    out = pool.solve(None, 4)  # a horizon's stacks are smaller: the whole pool fits, and the pool still solves
    assert (out[3] == 0).all() and (out[0] == 0).all() and (out[2] == 0).all()
    pool.close()


def test_a_running_position_without_a_legal_action_sets_the_error_word():
    """A full TicTacToe board without a line, marked as running, is no position of the game."""
    pool = DevicePool("TicTacToe", 4, seed=1)
    pool.reset(np.arange(4, dtype=np.int32))
    pool.recv_dict()
    row = pool.get_state([2])
    row[0, 2:11] = [0, 1, 0, 0, 1, 1, 1, 0, 0]
    pool.set_state(row, [2])
    with pytest.raises(RuntimeError, match="solve met a position that is no position of the game"):
        pool.solve([1, 2])
    pool.close()


def teardown_module(module):
    for c in _ctx.values():
        c.pool.close()
    _ctx.clear()
