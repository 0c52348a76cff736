"""The proven values of the PGX guided search on the MI355X: the PROVE forms of PgxGuidedAdvance, PgxGuidedAdvanceWide,
PgxGuidedResult and PgxGuidedReroot and PgxGuidedProof against the host harness of the same header
(tests/cpu_harness/pgx_prove_host.cpp) -- all emitted arrays, the result, `proof` and `decided` after every call, for
the four root sets of the CPU tests (pgx_prove_util.root_set: at most 16 roots, set into a pool with set_state), W in
{1, 4}, D in {0, 2}, with reroots, through DevicePool, env.guided_search and torch_interop.guided_search_device; a
2-shard pool; permuted and repeated ids; prove=False against a session opened without the parameter; and the refusals,
which come before any launch."""
import ctypes

import numpy as np
import pytest

import envpool_amd as envpool
import pgx_prove_util as U
import pgx_tactics_util as T
from envpool_amd.core import native
from envpool_amd.core.device_pool import DevicePool
from pgx_guided_util import stand_in

pytestmark = pytest.mark.gpu

F = np.float32
C_PUCT = U.C_PUCT
WIDE = 4
DEPTHS = (0, 2)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    return U.build_libs(tmp_path_factory.mktemp("pgx_prove_gpu"))


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
        assert k <= 16
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

    def host(self, libs, S, W, D, nodes=0, rows=None, flags=U.PROVE):
        roots = self.roots if rows is None else [self.roots[i] for i in rows]
        return U.ProveHost(libs, self.fam, roots, S, W, D, flags, U.BIG, nodes)


_ctx = {}


def get_ctx(libs, fam):
    if fam not in _ctx:
        _ctx[fam] = Ctx(libs, fam)
    return _ctx[fam]


def wide_rows(x, width):
    """Leaf arrays of a plain session with the slot axis the harness keeps."""
    return x if width else tuple(a[:, None] for a in x)


def run_against_harness(libs, ctx, width, depth, nodes=0, rows=None, reroots=0):
    """A prove session through the host forms and the harness's, fed the stand-in evaluator's rows, compared after
    every call: leaves, result, proof and decided.  Returns the record of the pool's session."""
    pool, S = ctx.pool, U.SIMS[ctx.fam]
    ids = ctx.ids if rows is None else np.asarray(rows, np.int32)
    W = width or 1
    host = ctx.host(libs, S, W, depth, nodes, rows)
    leaves = wide_rows(pool.guided_begin(ids, S, C_PUCT, nodes, width, depth, U.BIG, True), width)
    same(pool.guided_proof(), host.proof(), (ctx.fam, "begin"))
    rec = dict(leaves=[leaves], results=[], proofs=[])
    for move in range(reroots + 1):
        calls = 0
        while True:
            same(leaves, host.leaves(), (ctx.fam, width, depth, move, calls))
            # (a plain session keeps lockstep: its round has S + 1 advances even when every root is proven before)
            if (leaves[2] == 2).all() and (width or calls > S or move == reroots):
                break
            assert calls <= S
            priors, values = T.stand_in_rows(leaves[0], leaves[1])
            got = pool.guided_advance(priors if width else priors[:, 0], values if width else values[:, 0])
            leaves = wide_rows(got, width)
            assert host.advance(priors, values) == 0
            res, proof = pool.guided_result(), pool.guided_proof()
            same(res, host.result()[:3], (ctx.fam, width, depth, move, calls))
            same(proof, host.proof(), (ctx.fam, width, depth, move, calls))
            same((pool.guided_decided(),), (host.decided()[0],), (ctx.fam, width, depth, move, calls))
            rec["leaves"].append(leaves)
            rec["results"].append(res)
            rec["proofs"].append(proof)
            calls += 1
        if move < reroots:
            # by turns onto a child that is proven (a marked node, or a decided or finished one) and the chosen move
            value, q = pool.guided_proof()
            action = pool.guided_result()[2]
            sent = np.where(action < 0, 0, action).astype(np.int32)
            for i in range(len(sent)):
                known = np.flatnonzero(q[i] != U.UNPROVEN)
                if (i + move) % 2 == 0 and len(known):
                    sent[i] = known[0]
            leaves = wide_rows(pool.guided_reroot(sent, S - 2), width)
            assert host.reroot(sent, S - 2) == 0
            same(pool.guided_result(), host.result()[:3], (ctx.fam, "kept"))
            same(pool.guided_proof(), host.proof(), (ctx.fam, "reroot"))
            rec["proofs"].append(pool.guided_proof())
            S = S - 2
    pool.guided_end()
    host.close()
    assert np.array_equal(pool.get_state(), ctx.st)  # nothing of the pool changes
    return rec


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("fam", U.GAMES)
def test_kernels_equal_the_host_harness(libs, fam, wide):
    ctx = get_ctx(libs, fam)
    width = WIDE if wide else None
    for depth in DEPTHS:
        rec = run_against_harness(libs, ctx, width, depth)
        value, q = rec["proofs"][-1]
        assert value.dtype == np.int8 and value.shape == (ctx.k,) and q.dtype == np.int8
        assert q.shape == (ctx.k, ctx.pool.guided_shape()[3])
        assert (value != U.UNPROVEN).any() and set(np.unique(value).tolist()) <= {-128, -1, 0, 1}
        visits, _, action = rec["results"][-1]
        proven = value != U.UNPROVEN
        assert (visits[proven].sum(1) <= U.SIMS[fam]).all()
        assert (q[proven, action[proven]] == value[proven]).all()  # the move played keeps the proven value
        for lv in rec["leaves"]:
            idle = lv[2] != 0
            assert not lv[0][idle].any() and not lv[1][idle].any()


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("fam", U.GAMES)
def test_reroot_equals_the_harness(libs, fam, wide):
    """nodes = 3 S + 1 and two reroots, by turns onto proven children -- a marked node runs on as the new root and is
    proven at once -- and by the chosen moves."""
    ctx = get_ctx(libs, fam)
    at_once = 0
    for depth in DEPTHS:
        rec = run_against_harness(libs, ctx, WIDE if wide else None, depth, nodes=3 * U.SIMS[fam] + 1, reroots=2)
        at_once += sum(int((p[0] != U.UNPROVEN).sum()) for p in rec["proofs"])
    assert at_once > 0


@pytest.mark.parametrize("fam", ["ConnectFour", "Othello"])
def test_permuted_and_repeated_ids_give_the_same_rows(libs, fam):
    ctx = get_ctx(libs, fam)
    W, D = WIDE, 2
    base = run_against_harness(libs, ctx, W, D)
    rows = np.random.default_rng(4).permutation(ctx.k).astype(np.int32)
    rows[-1], rows[-2] = rows[0], rows[1]  # out of order, two ids twice
    other = run_against_harness(libs, ctx, W, D, rows=rows)
    assert len(base["leaves"]) == len(other["leaves"])
    for a, b in zip(base["leaves"], other["leaves"]):
        same([x[rows] for x in a], b)
    same([x[rows] for x in base["results"][-1]], other["results"][-1])
    same([x[rows] for x in base["proofs"][-1]], other["proofs"][-1])


@pytest.mark.parametrize("fam", U.GAMES)
def test_prove_false_equals_a_session_opened_without_the_parameter(libs, fam):
    """Through the new C entry point with flags = 0, plain, wide and with tactics, against guided_begin as it was; and
    the read-out of such a session is -128 everywhere."""
    ctx = get_ctx(libs, fam)
    pool, S, k = ctx.pool, U.SIMS[fam], ctx.k
    h, w, c, a = pool.guided_shape()
    for width, D in ((0, 0), (WIDE, 0), (WIDE, 2)):
        n = k * max(width, 1)

        def raw_begin():
            obs, mask = np.zeros((n, h, w, c), np.bool_), np.zeros((n, a), np.bool_)
            status = np.zeros(n, np.uint8)
            native.check(pool._lib.epa_guided_begin_prove(pool._h, ctx.ids.ctypes.data, k, S, 0, width,
                                                          ctypes.c_float(C_PUCT), D, U.BIG, 0, obs.ctypes.data,
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
                rec.append(list(pool.guided_result()) + [pool.guided_decided()])
                value, q = pool.guided_proof()
                assert (value == U.UNPROVEN).all() and (q == U.UNPROVEN).all()
            return rec

        old = session(lambda: pool.guided_begin(ctx.ids, S, C_PUCT, 0, width or None, D, U.BIG))
        new = session(raw_begin)
        also = session(lambda: pool.guided_begin(ctx.ids, S, C_PUCT, 0, width or None, D, U.BIG, False))
        pool.guided_end()
        assert len(old) == len(new) == len(also)
        for x, y, z in zip(old, new, also):
            same(x, y, (fam, width))
            same(x, z, (fam, width))


def _stepped_env(fam, device, plies):
    env = envpool.make(f"{fam}-v1", "gymnasium", num_envs=16, device=device, seed=11)
    rng = np.random.default_rng(2)
    _, info = env.reset()
    for _ in range(plies):
        mask = np.asarray(info["legal_action_mask"], bool)
        _, _, _, _, info = env.step((rng.random(mask.shape) * mask + mask).argmax(1).astype(np.int32))
    return env


@pytest.mark.parametrize("width", [1, 4])
def test_env_guided_search_and_a_sharded_pool(libs, width):
    """env.guided_search(prove=True) on TicTacToe 3 plies in: the unsharded pool against the harness fed its own state
    rows, and a 2-shard pool (the second shard with env_id_offset 8) against the unsharded rows."""
    fam, S, D = "TicTacToe", 32, 2
    ids = np.array([13, 3, 15, 0, 8, 7, 3, 12, 5, 10], np.int32)  # both shards, out of order, id 3 twice
    results = []
    for device in (0, [0, 0]):
        env = _stepped_env(fam, device, 3)
        gs = env.guided_search(ids, simulations=S, c_puct=C_PUCT, nodes=2 * S + 1, width=width, tactics=D,
                               tactics_nodes=U.BIG, prove=True)
        assert gs.prove is True and (gs.proof.value == U.UNPROVEN).all()
        rec = []
        host = None
        if device == 0:
            st = env.device_pool.get_state(ids)
            game = U.Game(libs, fam)
            roots = [game.pos(np.asarray(r[2:], np.int32), r[1] != 0) for r in st]
            host = U.ProveHost(libs, fam, roots, S, width, D, U.PROVE, U.BIG, 2 * S + 1)
        for move in range(2):
            while not gs.done or (width == 1 and gs.calls <= gs.simulations):  # (a plain round: S + 1 advances)
                leaves = gs.leaves
                lead = leaves[2].shape
                priors, values = T.stand_in_rows(leaves[0], leaves[1])
                if host is not None:
                    same([x.reshape(host.obs.shape[:2] + x.shape[len(lead):]) for x in leaves], host.leaves(), move)
                    assert host.advance(priors.reshape(len(ids), width, -1), values.reshape(len(ids), width)) == 0
                gs.advance(priors, values)
                rec.append([np.asarray(x).copy() for x in gs.leaves] + list(gs.result()) + list(gs.proof))
                if host is not None:
                    same(rec[-1][3:6], host.result()[:3], move)
                    same(rec[-1][6:8], host.proof(), move)
            action = gs.result().action
            sent = np.where(action < 0, 0, action).astype(np.int32)
            gs.reroot(sent)
            if host is not None:
                assert host.reroot(sent, S) == 0
            rec.append([np.asarray(x).copy() for x in gs.leaves] + list(gs.result()) + list(gs.proof))
            if host is not None:
                same(rec[-1][6:8], host.proof(), "reroot")
        gs.close()
        if host is not None:
            host.close()
        results.append(rec)
        env.close()
    assert len(results[0]) == len(results[1])
    assert any((r[6] != U.UNPROVEN).any() for r in results[0])  # roots were proven on the way
    for x, y in zip(*results):
        same(x, y)


@pytest.mark.parametrize("fam", ["TicTacToe", "Othello"])
def test_device_form_with_advances_given(libs, fam):
    """guided_search_device(width=, tactics=, prove=True, advances=): no host wait; the evaluator's rows are recorded on
    the way and fed to the harness, whose result and proofs the device tensors equal; then guided_reroot_device."""
    import torch

    from envpool_amd.torch_interop import guided_proof_device, guided_reroot_device, guided_search_device

    ctx = get_ctx(libs, fam)
    pool, S, W, D, k = ctx.pool, U.SIMS[fam], WIDE, 2, ctx.k
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
                                 advances=calls, tactics=D, tactics_nodes=U.BIG, prove=True)
    value, q = guided_proof_device(pool)
    read()
    assert value.is_cuda and value.dtype == torch.int8 and value.shape == (k,) and q.shape == (k, a)
    assert len(fed) == calls
    host = ctx.host(libs, S, W, D, nodes)
    for priors, values, status in fed:
        same((status.reshape(k, W),), (host.status,))
        assert host.advance(priors.reshape(k, W, a), values.reshape(k, W)) == 0
    same([t.cpu().numpy() for t in first], host.result()[:3], fam)
    same((value.cpu().numpy(), q.cpu().numpy()), host.proof(), fam)
    assert (value.cpu().numpy() != U.UNPROVEN).any()
    if (host.status == 2).all():
        actions = torch.where(first[2] < 0, torch.zeros_like(first[2]), first[2])
        second = guided_reroot_device(pool, evaluate, actions, S - 2, advances=3)
        read()
        assert host.reroot(actions.cpu().numpy(), S - 2) == 0
        for priors, values, status in fed:
            same((status.reshape(k, W),), (host.status,))
            assert host.advance(priors.reshape(k, W, a), values.reshape(k, W)) == 0
        same([t.cpu().numpy() for t in second], host.result()[:3], (fam, "second"))
        same([t.cpu().numpy() for t in guided_proof_device(pool)], host.proof(), (fam, "second"))
    pool.guided_end()
    host.close()
    assert np.array_equal(pool.get_state(), ctx.st)


def _raw_begin(pool, ids, S, nodes, width, tactics, m, flags, device=False):
    ids = np.ascontiguousarray(ids, np.int32)
    h, w, c, a = pool.guided_shape()
    n = max(len(ids), 1) * max(min(width, 32), 1)
    obs, mask, status = np.zeros((n, h, w, c), np.uint8), np.zeros((n, a), np.uint8), np.zeros(n, np.uint8)
    fn = pool._lib.epa_guided_begin_prove_device if device else pool._lib.epa_guided_begin_prove
    native.check(fn(pool._h, ids.ctypes.data, len(ids), S, nodes, width, ctypes.c_float(C_PUCT), tactics, m, flags,
                    obs.ctypes.data, mask.ctypes.data, status.ctypes.data))


def test_refusals_come_before_any_launch(libs):
    cart = DevicePool("CartPole", 4, seed=1)
    buf = np.zeros(4096, np.int32)
    with pytest.raises(RuntimeError, match="guided search not implemented"):
        native.check(cart._lib.epa_guided_begin_prove(cart._h, buf.ctypes.data, 2, 8, 0, 0, ctypes.c_float(1.0), 0,
                                                      4096, 1, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data))
    with pytest.raises(RuntimeError, match="guided search not implemented"):
        cart.guided_begin(None, 8, C_PUCT, 0, None, 0, 4096, True)
    cart.close()
    ctx = get_ctx(libs, "ConnectFour")
    pool = ctx.pool
    if getattr(pool, "_guided_k", None) is not None:
        pool.guided_end()
    with pytest.raises(ValueError, match="no guided-search session"):
        pool.guided_proof()
    for bad in (1, "yes", 2.0):
        with pytest.raises(ValueError, match="guided_begin: prove"):
            pool.guided_begin(ctx.ids, 8, C_PUCT, 0, None, 0, 4096, bad)
    for device in (False, True):
        for width in (0, 4):
            for flags in (2, 3, -1):
                with pytest.raises(ValueError, match="guided_begin: flags"):
                    _raw_begin(pool, ctx.ids, 8, 0, width, 0, 4096, flags, device)
            with pytest.raises(ValueError, match="guided_begin: tactics"):
                _raw_begin(pool, ctx.ids, 8, 0, width, 17, 4096, 1, device)
    with pytest.raises(ValueError, match="guided_begin: width"):
        _raw_begin(pool, ctx.ids, 8, 0, 33, 0, 64, 1)
    with pytest.raises(ValueError, match="no guided-search session"):  # none of them opened one
        pool.guided_end()
    env = envpool.make("ConnectFour-v1", "gymnasium", num_envs=4, seed=1)
    env.reset()
    for call in (lambda: env.guided_search(simulations=8, prove=1),
                 lambda: env.gumbel_search(simulations=8, prove=True),
                 lambda: env.guided_search(simulations=8, policy="gumbel", prove=True)):
        with pytest.raises(ValueError, match="prove"):
            call()
    # a Gumbel session has no proofs
    gs = env.gumbel_search(simulations=4, seed=1)
    with pytest.raises(ValueError, match="gumbel|Gumbel"):
        env.device_pool.guided_proof()
    gs.close()
    env.close()
