"""The exact leaf status of the PGX guided search on the MI355X: PgxGuidedTactics behind PgxGuidedAdvance and
PgxGuidedAdvanceWide, and the reroot that reopens a decided root, against the host harness of the same header
(tests/cpu_harness/pgx_tactics_host.cpp) -- all emitted arrays, the result and `decided` after every call, for the four
root sets of the CPU tests (pgx_tactics_util.root_set: at most 12 roots, set into a pool with set_state), through
DevicePool, env.guided_search and torch_interop.guided_search_device; a sharded pool; permuted and repeated ids;
tactics = 0 against a session opened without the parameter; and the refusals, which come before any launch."""
import ctypes

import numpy as np
import pytest

import envpool_amd as envpool
import pgx_tactics_util as U
from envpool_amd.core import native
from envpool_amd.core.device_pool import DevicePool
from pgx_guided_util import stand_in

pytestmark = pytest.mark.gpu

F = np.float32
C_PUCT = U.C_PUCT


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pgx_tactics_gpu")
    out = U.build_libs(tmp)
    out["guided"] = ctypes.CDLL(U.compile_harness(tmp, "pgx_guided_host.cpp"))
    return out


def same(a, b, what=None):
    """Two tuples of arrays, bit for bit (floats by their bits, bools as bytes)."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.shape == y.shape, (what, x.shape, y.shape)
        assert x.dtype.itemsize == y.dtype.itemsize, (what, x.dtype, y.dtype)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), what


class Ctx:
    """One pool per game holding the game's root set, one env per root."""

    def __init__(self, libs, fam):
        self.fam, self.game = fam, U.Game(libs, fam)
        self.roots = U.root_set(libs, self.game)
        self.k = k = len(self.roots)
        assert k <= 12
        self.pool = pool = DevicePool(fam, k, seed=11)
        self.ids = np.arange(k, dtype=np.int32)
        pool.reset(self.ids)
        pool.recv_dict()
        rows = pool.get_state()
        for i, r in enumerate(self.roots):
            rows[i, 0], rows[i, 1], rows[i, 2:] = 1.0, float(r.done), r.key[1]
        pool.set_state(rows, self.ids)
        self.st = pool.get_state()
        assert np.array_equal(self.st[:, 1:], rows[:, 1:])

    def host(self, libs, S, W, D, M=U.BIG, nodes=0, rows=None):
        roots = self.roots if rows is None else [self.roots[i] for i in rows]
        return U.TacticsHost(libs, self.fam, roots, S, W, D, M, nodes)


_ctx = {}


def get_ctx(libs, fam):
    if fam not in _ctx:
        _ctx[fam] = Ctx(libs, fam)
    return _ctx[fam]


def wide_rows(x, width):
    """Leaf arrays of a plain session with the slot axis the harness keeps."""
    return x if width else tuple(a[:, None] for a in x)


def run_against_harness(libs, ctx, width, depth, M=U.BIG, nodes=0, begin=None, rows=None, reroots=0):
    """A session through the host forms and the harness's, fed the stand-in evaluator's rows, compared after every
    call: leaves, result, decided and the solver's visited positions.  Returns the record of the pool's session."""
    pool, S = ctx.pool, U.SIMS[ctx.fam]
    ids = ctx.ids if rows is None else np.asarray(rows, np.int32)
    W = width or 1
    host = ctx.host(libs, S, W, depth, M, nodes, rows)
    begin = begin or (lambda: pool.guided_begin(ids, S, C_PUCT, nodes, width, depth, M))
    leaves = wide_rows(begin(), width)
    rec = dict(leaves=[leaves], results=[], decided=[])
    for move in range(reroots + 1):
        calls = 0
        while True:
            same(leaves, host.leaves(), (ctx.fam, width, depth, move, calls))
            if (leaves[2] == 2).all():
                break
            assert calls <= S
            priors, values = U.stand_in_rows(leaves[0], leaves[1])
            got = pool.guided_advance(priors if width else priors[:, 0], values if width else values[:, 0])
            leaves = wide_rows(got, width)
            assert host.advance(priors, values) == 0
            res, (decided, nodes_seen) = pool.guided_result(), pool.guided_decided(with_nodes=True)
            same(res, host.result()[:3], (ctx.fam, width, depth, move, calls))
            want = host.decided()
            same((decided, nodes_seen), want[:2], (ctx.fam, width, depth, move, calls, decided, want[0]))
            rec["leaves"].append(leaves)
            rec["results"].append(res)
            rec["decided"].append(decided)
            calls += 1
        if move < reroots:
            action = pool.guided_result()[2]
            sent = np.where(action < 0, 0, action).astype(np.int32)
            leaves = wide_rows(pool.guided_reroot(sent, S - 2), width)
            assert host.reroot(sent, S - 2) == 0
            same(pool.guided_result(), host.result()[:3], (ctx.fam, "kept"))
            same((pool.guided_decided(),), (host.decided()[0],), (ctx.fam, "reroot keeps the counters"))
            S = S - 2
    pool.guided_end()
    host.close()
    assert np.array_equal(pool.get_state(), ctx.st)  # nothing of the pool changes
    return rec


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("fam", U.GAMES)
def test_kernels_equal_the_host_harness(libs, fam, wide):
    ctx = get_ctx(libs, fam)
    width = U.WIDTH[fam] if wide else None
    statuses = set()
    for depth in U.DEPTHS[fam]:
        rec = run_against_harness(libs, ctx, width, depth)
        obs, mask, status = rec["leaves"][0]
        assert obs.dtype == np.bool_ and mask.dtype == np.bool_ and status.dtype == np.uint8
        assert rec["decided"][-1].dtype == np.int32 and rec["decided"][-1].shape == (ctx.k,)
        assert rec["decided"][-1].sum() > 0
        for lv in rec["leaves"]:
            statuses |= set(np.unique(lv[2]).tolist())
            idle = lv[2] != 0
            assert not lv[0][idle].any() and not lv[1][idle].any()  # a decided row is zeros, like a finished game's
    assert statuses == {0, 1, 2}


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("fam", ["TicTacToe", "ConnectFour"])
def test_reroot_equals_the_harness(libs, fam, wide):
    """nodes = 3 S + 1 and two reroots by the chosen moves -- in TicTacToe at D = 2 the most visited move often leads to
    a decided child, which runs on as the new root."""
    ctx = get_ctx(libs, fam)
    rec = run_against_harness(libs, ctx, U.WIDTH[fam] if wide else None, 2, nodes=3 * U.SIMS[fam] + 1, reroots=2)
    assert (rec["decided"][-1] >= rec["decided"][0]).all()


def test_a_tight_budget_equals_the_harness(libs):
    """M = 64 on ConnectFour at D = 4: the given-up leaves are the harness's, so the sessions agree call for call."""
    ctx = get_ctx(libs, "ConnectFour")
    tight = run_against_harness(libs, ctx, 4, 4, M=64)
    roomy = run_against_harness(libs, ctx, 4, 4)
    assert roomy["decided"][-1].sum() > tight["decided"][-1].sum()


@pytest.mark.parametrize("fam", ["ConnectFour", "Othello"])
def test_permuted_and_repeated_ids_give_the_same_rows(libs, fam):
    ctx = get_ctx(libs, fam)
    W, D = U.WIDTH[fam], 2
    base = run_against_harness(libs, ctx, W, D)
    rows = np.random.default_rng(4).permutation(ctx.k).astype(np.int32)
    rows[-1], rows[-2] = rows[0], rows[1]  # out of order, two ids twice
    other = run_against_harness(libs, ctx, W, D, rows=rows)
    assert len(base["leaves"]) == len(other["leaves"])
    for a, b in zip(base["leaves"], other["leaves"]):
        same([x[rows] for x in a], b)
    same([x[rows] for x in base["results"][-1]], other["results"][-1])
    same((base["decided"][-1][rows],), (other["decided"][-1],))


@pytest.mark.parametrize("fam", U.GAMES)
def test_tactics_0_equals_a_session_opened_without_the_parameter(libs, fam):
    """Through the new C entry point with tactics = 0, plain and wide, against guided_begin as it was."""
    ctx = get_ctx(libs, fam)
    pool, S, k = ctx.pool, U.SIMS[fam], ctx.k
    h, w, c, a = pool.guided_shape()
    for width in (0, U.WIDTH[fam]):
        n = k * max(width, 1)

        def raw_begin():
            obs, mask = np.zeros((n, h, w, c), np.bool_), np.zeros((n, a), np.bool_)
            status = np.zeros(n, np.uint8)
            native.check(pool._lib.epa_guided_begin_tactics(pool._h, ctx.ids.ctypes.data, k, S, 0, width,
                                                            ctypes.c_float(C_PUCT), 0, 4096, obs.ctypes.data,
                                                            mask.ctypes.data, status.ctypes.data))
            return obs, mask, status

        def session(begin):
            leaves, rec = begin(), []
            for _ in range(S + 1):
                flat = [np.ascontiguousarray(leaves[0]).reshape(n, h, w, c),
                        np.ascontiguousarray(leaves[1]).reshape(n, a), np.ascontiguousarray(leaves[2]).reshape(n)]
                rec.append([x.copy() for x in flat])
                priors, values = stand_in(flat[0], flat[1])
                if width:
                    priors, values = priors.reshape(k, width, a), values.reshape(k, width)
                leaves = pool.guided_advance(priors, values)
                rec.append(list(pool.guided_result()))
            return rec

        old = session(lambda: pool.guided_begin(ctx.ids, S, C_PUCT, 0, width or None))
        assert not pool.guided_decided().any()
        new = session(raw_begin)
        decided, nodes = pool.guided_decided(with_nodes=True)
        assert not decided.any() and not nodes.any()
        pool.guided_end()
        assert len(old) == len(new)
        for x, y in zip(old, new):
            same(x, y, (fam, width))


def _stepped_env(fam, device, plies):
    env = envpool.make(f"{fam}-v1", "gymnasium", num_envs=24, device=device, seed=11)
    rng = np.random.default_rng(2)
    _, info = env.reset()
    for _ in range(plies):
        mask = np.asarray(info["legal_action_mask"], bool)
        _, _, _, _, info = env.step((rng.random(mask.shape) * mask + mask).argmax(1).astype(np.int32))
    return env


@pytest.mark.parametrize("width", [1, 4])
def test_env_guided_search_and_a_sharded_pool(libs, width):
    """env.guided_search(tactics=) on ConnectFour 10 plies in: the unsharded pool against the harness fed its own state
    rows, and a 2-shard pool (the second shard with env_id_offset 12) against the unsharded rows."""
    fam, S, D = "ConnectFour", 24, 2
    ids = np.array([17, 3, 23, 0, 12, 11, 3, 20, 8, 14], np.int32)  # both shards, out of order, id 3 twice
    results = []
    for device in (0, [0, 0]):
        env = _stepped_env(fam, device, 10)
        gs = env.guided_search(ids, simulations=S, c_puct=C_PUCT, nodes=2 * S + 1, width=width, tactics=D,
                               tactics_nodes=U.BIG)
        assert gs.tactics == D and not gs.decided.any()
        rec = []
        host = None
        if device == 0:
            st = env.device_pool.get_state(ids)
            game = U.Game(libs, fam)
            roots = [game.pos(np.asarray(r[2:], np.int32), r[1] != 0) for r in st]
            host = U.TacticsHost(libs, fam, roots, S, width, D, U.BIG, 2 * S + 1)
        for move in range(2):
            while not gs.done:
                leaves = gs.leaves
                lead = leaves[2].shape
                priors, values = U.stand_in_rows(leaves[0], leaves[1])
                if host is not None:
                    same([x.reshape(host.obs.shape[:2] + x.shape[len(lead):]) for x in leaves], host.leaves(), move)
                    assert host.advance(priors.reshape(len(ids), width, -1), values.reshape(len(ids), width)) == 0
                gs.advance(priors, values)
                rec.append([np.asarray(x).copy() for x in gs.leaves] + list(gs.result()) + [gs.decided])
                if host is not None:
                    same(rec[-1][3:6], host.result()[:3], move)
                    same((rec[-1][6],), (host.decided()[0],), move)
            action = gs.result().action
            sent = np.where(action < 0, 0, action).astype(np.int32)
            gs.reroot(sent)
            if host is not None:
                assert host.reroot(sent, S) == 0
            rec.append([np.asarray(x).copy() for x in gs.leaves] + list(gs.result()) + [gs.decided])
        gs.close()
        if host is not None:
            host.close()
        results.append(rec)
        env.close()
    assert len(results[0]) == len(results[1]) and results[0][-1][6].sum() > 0
    for x, y in zip(*results):
        same(x, y)


@pytest.mark.parametrize("fam", ["TicTacToe", "Othello"])
def test_device_form_with_advances_given(libs, fam):
    """guided_search_device(width=, tactics=, advances=): no host wait; the evaluator's rows are recorded on the way and
    fed to the harness, whose result and counters the device tensors equal; then guided_reroot_device."""
    import torch

    from envpool_amd.torch_interop import guided_decided_device, guided_reroot_device, guided_search_device

    ctx = get_ctx(libs, fam)
    pool, S, W, D, k = ctx.pool, U.SIMS[fam], U.WIDTH[fam], 2, ctx.k
    a = pool.guided_shape()[3]
    dev = torch.device("cuda", pool.device)
    n_obs = int(np.prod(U.SHAPE[fam]))
    gen = torch.Generator().manual_seed(3)
    w_p = (torch.randn((n_obs, a), generator=gen) * 0.3).to(dev)
    w_v = (torch.randn((n_obs,), generator=gen) * 0.2).to(dev)
    kept, fed = [], []

    def evaluate(obs, mask, status):  # all on the device: what it returns and saw is read after the search
        assert obs.is_cuda and status.dtype == torch.uint8 and status.shape == (k * W,)
        x = obs.reshape(obs.shape[0], -1).float()
        priors, values = torch.softmax(x @ w_p, dim=1) * mask.float(), torch.tanh(x @ w_v)
        kept.append((priors, values, status.clone()))
        return priors, values

    def read():
        fed[:] = [tuple(t.cpu().numpy() for t in row) for row in kept]
        del kept[:]

    calls = S // 2
    nodes = 2 * S + 1
    first = guided_search_device(pool, evaluate, ctx.ids, S, C_PUCT, nodes=nodes, keep_open=True, width=W,
                                 advances=calls, tactics=D, tactics_nodes=U.BIG)
    decided = guided_decided_device(pool)
    read()
    assert decided.is_cuda and decided.dtype == torch.int32 and decided.shape == (k,) and len(fed) == calls
    host = ctx.host(libs, S, W, D, U.BIG, nodes)
    for priors, values, status in fed:
        same((status.reshape(k, W),), (host.status,))
        assert host.advance(priors.reshape(k, W, a), values.reshape(k, W)) == 0
    same([t.cpu().numpy() for t in first], host.result()[:3], fam)
    same((decided.cpu().numpy(),), (host.decided()[0],), fam)
    assert (np.concatenate([f[2] for f in fed]) == 1).any()  # the evaluator saw decided or finished rows
    if (host.status == 2).all():
        actions = torch.where(first[2] < 0, torch.zeros_like(first[2]), first[2])
        second = guided_reroot_device(pool, evaluate, actions, S - 2, advances=3)
        read()
        assert host.reroot(actions.cpu().numpy(), S - 2) == 0
        for priors, values, status in fed:
            same((status.reshape(k, W),), (host.status,))
            assert host.advance(priors.reshape(k, W, a), values.reshape(k, W)) == 0
        same([t.cpu().numpy() for t in second], host.result()[:3], (fam, "second"))
        same((guided_decided_device(pool).cpu().numpy(),), (host.decided()[0],))
    pool.guided_end()
    host.close()
    assert np.array_equal(pool.get_state(), ctx.st)


def _raw_begin(pool, ids, S, nodes, width, tactics, m, device=False):
    ids = np.ascontiguousarray(ids, np.int32)
    h, w, c, a = pool.guided_shape()
    n = max(len(ids), 1) * max(min(width, 32), 1)
    obs, mask, status = np.zeros((n, h, w, c), np.uint8), np.zeros((n, a), np.uint8), np.zeros(n, np.uint8)
    fn = pool._lib.epa_guided_begin_tactics_device if device else pool._lib.epa_guided_begin_tactics
    native.check(fn(pool._h, ids.ctypes.data, len(ids), S, nodes, width, ctypes.c_float(C_PUCT), tactics, m,
                    obs.ctypes.data, mask.ctypes.data, status.ctypes.data))


def test_refusals_come_before_any_launch(libs):
    cart = DevicePool("CartPole", 4, seed=1)
    buf = np.zeros(4096, np.int32)
    with pytest.raises(RuntimeError, match="guided search not implemented"):
        native.check(cart._lib.epa_guided_begin_tactics(cart._h, buf.ctypes.data, 2, 8, 0, 0, ctypes.c_float(1.0), 2,
                                                        4096, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data))
    with pytest.raises(RuntimeError, match="guided search not implemented"):
        cart.guided_begin(None, 8, C_PUCT, 0, None, 2)
    cart.close()
    ctx = get_ctx(libs, "ConnectFour")
    pool = ctx.pool
    if getattr(pool, "_guided_k", None) is not None:
        pool.guided_end()
    for tactics, m in ((17, 4096), (-1, 4096), (2, 0), (2, (1 << 20) + 1)):
        with pytest.raises(ValueError, match="guided_begin: tactics"):
            pool.guided_begin(ctx.ids, 8, C_PUCT, 0, None, tactics, m)
        for device in (False, True):
            for width in (0, 4):
                with pytest.raises(ValueError, match="guided_begin: tactics"):
                    _raw_begin(pool, ctx.ids, 8, 0, width, tactics, m, device)
    with pytest.raises(ValueError, match="guided_begin: width"):
        _raw_begin(pool, ctx.ids, 8, 0, 33, 2, 64)
    with pytest.raises(ValueError, match="no guided-search session"):  # none of them opened one
        pool.guided_end()
    env = envpool.make("ConnectFour-v1", "gymnasium", num_envs=4, seed=1)
    env.reset()
    for call in (lambda: env.guided_search(simulations=8, tactics=17),
                 lambda: env.guided_search(simulations=8, tactics=2, tactics_nodes=0),
                 lambda: env.gumbel_search(simulations=8, tactics=2),
                 lambda: env.guided_search(simulations=8, policy="gumbel", tactics=2)):
        with pytest.raises(ValueError, match="tactics"):
            call()
    # a Gumbel session has no counters
    gs = env.gumbel_search(simulations=4, seed=1)
    with pytest.raises(ValueError, match="gumbel|Gumbel"):
        env.device_pool.guided_decided()
    gs.close()
    env.close()


def test_a_begin_past_the_tree_limit_names_the_largest_k(libs):
    """Hex, nodes = 8192, width = 32, D = 16: the trees, the wide records and the stacks of one root, against 2 GiB."""
    g = libs["guided"]
    per_root = (8192 * g.pgx_guided_node_bytes(U.CODE["Hex"]) + libs["tactics"].pgx_wide_root_bytes(32)
                + 32 * 5120 * 16)
    fits = (2**31) // per_root
    without = (2**31) // (per_root - 32 * 5120 * 16)
    assert fits < without  # the stacks count
    pool = DevicePool("Hex", without, seed=3)
    ids = np.arange(without, dtype=np.int32)
    pool.reset(ids)
    pool.recv_dict()
    with pytest.raises(ValueError, match=f"at most {fits} roots fit"):
        pool.guided_begin(ids[: fits + 1], 8, C_PUCT, 8192, 32, 16, 64)
    with pytest.raises(ValueError, match=f"at most {fits} roots fit"):
        _raw_begin(pool, ids[: fits + 1], 8, 8192, 32, 16, 64, device=True)
    with pytest.raises(ValueError, match="no guided-search session"):  # it allocated and launched nothing
        pool.guided_end()
    pool.close()
