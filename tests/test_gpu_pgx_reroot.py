"""Tree reuse of the PGX guided search on the MI355X: PgxGuidedReroot and the capacity rule of PgxGuidedAdvance against
the host harness of the same header (tests/cpu_harness/pgx_reroot_host.cpp) fed the pool's own hidden words, the same
evaluator's numbers and the same played moves, for all four games -- leaves after every call and every reroot, results
after every round and every reroot; against the pool itself, stepped by the played moves; a fresh begin on the stepped
pool for moves the search never tried; sharding; the device form with a torch model; the move loop over a whole game;
the refusals and the session's life cycle.

The shape: a pool of 70 envs a few plies into their games with one env marked over, 11 ids out of order with one of
them twice (11 blocks of one wave), S = 24 simulations (Hex: S = 12), three moves, at nodes = 2 S + 1 and at
nodes = S + 1, where the rerooted trees run out of memory; and 3 roots at the capacities of the kernel's two larger
tables (513, 2049, 8192 nodes)."""
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
N, POOL_SEED, C_PUCT, MOVES = 70, 11, 1.25, 3
SIMS = {"TicTacToe": 24, "ConnectFour": 24, "Hex": 12, "Othello": 24}
PRE = {"TicTacToe": 2, "ConnectFour": 3, "Hex": 3, "Othello": 3}
SHAPE = {"TicTacToe": (3, 3, 2), "ConnectFour": (6, 7, 2), "Hex": (11, 11, 4), "Othello": (8, 8, 2)}
OVER = 33  # the env marked over
IDS = np.array([41, 7, 69, OVER, 0, 64, 12, 63, 7, 50, 22], np.int32)  # out of order, id 7 twice
ROW_UNTRIED, ROW_LAST, ROW_HIGH = 4, 6, 9  # rows with a move of their own (below)
FIRST = [j for j, e in enumerate(IDS) if e not in IDS[:j]]  # the first row of every env
ALL = np.arange(N, dtype=np.int32)
F = np.float32


def legal_random(mask, rng):
    mask = np.asarray(mask, bool)
    return (rng.random(mask.shape) * mask + mask).argmax(1).astype(np.int32)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pgx_reroot") / "libpgxreroothost.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "cpu_harness", "pgx_reroot_host.cpp"), "-o", out], check=True)
    lib = ctypes.CDLL(out)
    lib.pgx_reroot_begin.restype = ctypes.c_void_p
    lib.pgx_reroot_result.restype = None
    lib.pgx_reroot_end.restype = None
    return lib


class Host:
    """The harness's session on rows of get_state ([cur_step, done, hidden words])."""

    def __init__(self, lib, fam, st, simulations, nodes, c_puct):
        self.lib, self.k, self.n_act = lib, len(st), ACTIONS[fam]
        hid = np.ascontiguousarray(st[:, 2:], np.int32)
        done = np.ascontiguousarray(st[:, 1] != 0, np.uint8)
        self.obs = np.full((self.k,) + SHAPE[fam], 7, np.uint8)
        self.mask, self.status = np.full((self.k, self.n_act), 7, np.uint8), np.full(self.k, 7, np.uint8)
        rc = ctypes.c_int(-9)
        self.h = lib.pgx_reroot_begin(CODE[fam], self.k, _ptr(hid), _ptr(done), simulations, nodes,
                                      ctypes.c_float(c_puct), _ptr(self.obs), _ptr(self.mask), _ptr(self.status),
                                      ctypes.byref(rc))
        assert rc.value == 0 and self.h

    def leaves(self):
        return self.obs.copy(), self.mask.copy(), self.status.copy()

    def advance(self, priors, values):
        priors, values = np.ascontiguousarray(priors, F), np.ascontiguousarray(values, F)
        assert self.lib.pgx_reroot_advance(ctypes.c_void_p(self.h), _ptr(priors), _ptr(values), _ptr(self.obs),
                                           _ptr(self.mask), _ptr(self.status)) == 0
        return self.leaves()

    def reroot(self, actions, simulations):
        actions = np.ascontiguousarray(actions, np.int32)
        assert self.lib.pgx_reroot_reroot(ctypes.c_void_p(self.h), _ptr(actions), simulations, _ptr(self.obs),
                                          _ptr(self.mask), _ptr(self.status)) == 0
        return self.leaves()

    def result(self):
        visits, values = np.full((self.k, self.n_act), -7, np.int32), np.full((self.k, self.n_act), -7, F)
        action, nodes = np.full(self.k, -7, np.int32), np.zeros(self.k, np.int32)
        self.lib.pgx_reroot_result(ctypes.c_void_p(self.h), _ptr(visits), _ptr(values), _ptr(action), _ptr(nodes))
        return (visits, values, action), nodes

    def close(self):
        self.lib.pgx_reroot_end(ctypes.c_void_p(self.h))


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


def rolled(fam, step):
    """PRE[fam] seeded random legal plies of every env through `step(actions) -> legal mask`."""
    rng = np.random.default_rng(2)
    mask = step(None)
    for _ in range(PRE[fam]):
        mask = step(legal_random(mask, rng))
    return mask


def evaluator(obs, mask):
    """The stand-in evaluator; row ROW_LAST calls every leaf good for the seat that moves there -- bad for the root's
    mover --, so that root keeps trying new moves and the last node made is a child of the root."""
    priors, values = stand_in(obs, mask)
    if len(values) > ROW_LAST:
        values[ROW_LAST] = 1.0
    return priors, values


def played(fam, before, after, root_mask):
    """The moves played after a round, from the results before and after its last advance: the most visited move on
    most rows (its subtree interleaves with dropped nodes), and on three rows
      ROW_UNTRIED  a legal move the search never tried (else the least visited): a fresh tree
      ROW_LAST     the move whose first visit the last advance backed up -- its child is the last node made, and it is
                   all that is kept (else a move visited once: one node kept, else the most visited)
      ROW_HIGH     Hex: the most visited cell >= 64, the second action slot of its lane."""
    visits, _, action = after
    acts = action.copy()
    notes = {}
    legal = root_mask[ROW_UNTRIED]
    if legal.any():
        cand = np.flatnonzero(legal)
        acts[ROW_UNTRIED] = cand[np.argmin(visits[ROW_UNTRIED][cand])]  # (ties: the lowest)
        notes["untried"] = visits[ROW_UNTRIED][acts[ROW_UNTRIED]] == 0
    if root_mask[ROW_LAST].any():
        new = np.flatnonzero((before[0][ROW_LAST] == 0) & (visits[ROW_LAST] == 1))
        once = np.flatnonzero(visits[ROW_LAST] == 1)
        if len(new):
            acts[ROW_LAST], notes["last"] = new[0], True
        elif len(once):
            acts[ROW_LAST] = once[0]
    if fam == "Hex" and root_mask[ROW_HIGH, 64:121].any():
        cand = 64 + np.flatnonzero(root_mask[ROW_HIGH, 64:121])
        acts[ROW_HIGH] = cand[np.argmax(visits[ROW_HIGH][cand])]
        notes["high"] = True
    return acts.astype(np.int32), notes


class Ctx:
    """One pool per game, a few plies in, env OVER marked over, with its state and snapshot."""

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
        self.games = {}

    def game(self, nodes):
        """Three moves through the host forms with reroot between the rounds, the pool stepped by the played moves.
        Records everything: per move the leaves before every call and after the last, the rows fed, the results
        before and after the last advance, the moves, the leaves reroot emitted, the result after reroot, and what the
        pool returned for the step."""
        if nodes in self.games:
            return self.games[nodes]
        pool, fam, S = self.pool, self.fam, SIMS[self.fam]
        log, notes = [], {}
        leaves = pool.guided_begin(IDS, S, C_PUCT, nodes)
        root_mask = leaves[1].copy()
        for move in range(MOVES):
            st = pool.get_state()
            rec = dict(leaves=[leaves], feed=[])
            for t in range(S + 1):
                rec["feed"].append(evaluator(leaves[0], leaves[1]))
                if t == S:
                    rec["before"] = pool.guided_result()
                leaves = pool.guided_advance(*rec["feed"][-1])
                rec["leaves"].append(leaves)
            rec["after"] = pool.guided_result()
            rec["acts"], n = played(fam, rec["before"], rec["after"], root_mask)
            notes.update({k: v or notes.get(k, False) for k, v in n.items()})
            # rows of roots that are over have action -1: the engine's host form wants 0 .. A-1, and ignores the row
            sent = np.where(rec["acts"] < 0, 0, rec["acts"]).astype(np.int32)
            leaves = pool.guided_reroot(sent, S)
            rec["sent"], rec["rerooted"], rec["kept"] = sent, leaves, pool.guided_result()
            assert np.array_equal(pool.get_state(), st), (fam, move)  # the search changes nothing in the pool
            # the move loop: the pool is stepped by the same moves (each env once; not the ones that are over)
            rows = [j for j in FIRST if root_mask[j].any()]
            pool.send(IDS[rows], sent[rows])
            out = pool.recv_dict()
            at = {int(e): j for j, e in zip(rows, IDS[rows])}
            rows = [at[int(e)] for e in out["info:env_id"]]  # (in the order recv gave them)
            assert len(rows) == len(at)
            rec["rows"], rec["out"] = rows, {k: np.asarray(v).copy() for k, v in out.items()}
            root_mask = leaves[1].copy()
            log.append(rec)
        pool.guided_end()
        pool.restore(self.S)
        assert np.array_equal(pool.get_state(), self.st) and np.array_equal(pool.snapshot(), self.S)
        self.games[nodes] = (log, notes)
        return self.games[nodes]


_ctx = {}


def get_ctx(fam):
    if fam not in _ctx:
        _ctx[fam] = Ctx(fam)
    return _ctx[fam]


@pytest.fixture(scope="module", params=GAMES)
def ctx(request):
    return get_ctx(request.param)


@pytest.mark.parametrize("roomy", [True, False])
def test_kernels_equal_the_host_harness_and_the_stepped_pool(ctx, harness, roomy):
    fam, S, n_act = ctx.fam, SIMS[ctx.fam], ACTIONS[ctx.fam]
    nodes = 2 * S + 1 if roomy else S + 1
    log, notes = ctx.game(nodes)
    host = Host(harness, fam, ctx.st[IDS], S, nodes, C_PUCT)
    over = ctx.st[IDS, 1] != 0
    twin = [j for j, e in enumerate(IDS) if e == 7]
    assert len(twin) == 2 and over[list(IDS).index(OVER)] and over.sum() == 1
    starved = False
    for move, rec in enumerate(log):
        want = host.leaves()
        for t in range(S + 1):
            same(rec["leaves"][t], want, (fam, move, t))
            want = host.advance(*rec["feed"][t])
        same(rec["leaves"][S + 1], want, (fam, move, "end"))
        assert (want[2] == 2).all()
        res, used = host.result()
        same(rec["after"], res, (fam, move))
        assert used.max() <= nodes
        starved = starved or (move > 0 and (used == nodes).any())
        running = rec["leaves"][0][2] == 0
        if move == 0 or (roomy and move == 1):  # (later the kept tree may use the memory up, even at 2 S + 1)
            assert (rec["after"][0][running].sum(1) >= S).all()  # the kept visits count
        visits = rec["after"][0]
        want = host.reroot(rec["sent"], S)
        same(rec["rerooted"], want, (fam, move, "reroot"))
        res, kept = host.result()
        same(rec["kept"], res, (fam, move, "kept"))
        obs, mask, status = rec["rerooted"]
        assert obs.dtype == np.bool_ and mask.dtype == np.bool_ and status.dtype == np.uint8
        assert set(np.unique(status)) <= {0, 2}
        still = status == 0
        # every simulation through the played edge but the one that made its child
        a = rec["sent"]
        rows = np.flatnonzero(still)
        through = visits[rows, a[rows]]
        assert np.array_equal(rec["kept"][0][rows].sum(1), np.maximum(through - 1, 0)), (fam, move)
        assert (kept[rows][through == 0] == 1).all() and (kept[rows][through == 1] == 1).all()
        assert (rec["kept"][2][~still] == -1).all() and not rec["kept"][0][~still].any()
        same([x[twin[0]] for x in rec["rerooted"]], [x[twin[1]] for x in rec["rerooted"]])
        # the pool, stepped by the same moves: its rows for the seat to move are the leaves reroot emitted
        out = rec["out"]
        mover = out["info:current_player"]
        obs_rows = out["obs"].reshape((len(rec["rows"]), 2) + obs.shape[1:])
        for i, j in enumerate(rec["rows"]):
            if out["done"][i]:
                assert status[j] == 2 and not obs[j].any() and not mask[j].any(), (fam, move, j)
            else:
                assert status[j] == 0, (fam, move, j)
                assert np.array_equal(obs[j], obs_rows[i, mover[i]]), (fam, move, j)
                assert np.array_equal(mask[j], out["info:legal_action_mask"][i]), (fam, move, j)
    host.close()
    if fam == "Hex":
        assert notes.get("untried") and notes.get("last") and notes.get("high"), notes
    if not roomy:
        assert starved, "the capacity did not bind"  # memory used up: a normal end, and still the harness


@pytest.mark.parametrize("fam,nodes", [("ConnectFour", 513), ("ConnectFour", 2049), ("ConnectFour", 8192),
                                       ("Hex", 513), ("Hex", 2049)])
def test_the_larger_reroot_tables_equal_the_harness(harness, fam, nodes):
    """PgxGuidedReroot with its 2048- and 8192-entry tables (capacities above 512 and above 2048), one and two action
    slots per lane: 3 roots, a round of 8 simulations, a reroot by the chosen moves and a second round -- leaves after
    every call, results after both rounds and after the reroot, bit for bit."""
    ctx = get_ctx(fam)
    pool, S, ids = ctx.pool, 8, IDS[:3]
    assert OVER not in ids
    host = Host(harness, fam, ctx.st[ids], S, nodes, C_PUCT)
    leaves = pool.guided_begin(ids, S, C_PUCT, nodes)
    same(leaves, host.leaves(), (fam, "begin"))
    for move in range(2):
        for t in range(S + 1):
            feed = stand_in(leaves[0], leaves[1])
            leaves = pool.guided_advance(*feed)
            same(leaves, host.advance(*feed), (fam, move, t))
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


@pytest.mark.parametrize("fam", GAMES)
def test_reroot_by_untried_moves_equals_a_fresh_begin_on_the_stepped_pool(fam):
    """A round of 2 simulations leaves most root moves without a child.  Every root is rerooted by such a move, into a
    longer round; the pool is stepped by the same moves; a session begun on the stepped pool and fed the same numbers
    gives the same leaves and results."""
    ctx = get_ctx(fam)
    pool, S2 = ctx.pool, SIMS[fam]
    ids = np.array(sorted(set(IDS.tolist()) - {OVER}), np.int32)
    leaves = pool.guided_begin(ids, 2, C_PUCT, S2 + 1)
    root_mask = leaves[1].copy()
    for t in range(3):
        leaves = pool.guided_advance(*stand_in(leaves[0], leaves[1]))
    visits = pool.guided_result()[0]
    untried = root_mask & (visits == 0)
    assert untried.any(1).all()
    acts = (untried * np.arange(1, untried.shape[1] + 1)).argmax(1).astype(np.int32)  # the highest untried move
    got, feed = [pool.guided_reroot(acts, S2)], []
    assert (pool.guided_result()[0] == 0).all()
    for t in range(S2 + 1):
        feed.append(stand_in(got[-1][0], got[-1][1]))
        got.append(pool.guided_advance(*feed[-1]))
    res = pool.guided_result()
    pool.send(ids, acts)
    out = pool.recv_dict()
    assert np.array_equal(out["info:env_id"], ids)
    fresh = [pool.guided_begin(ids, S2, C_PUCT)]
    for t in range(S2 + 1):
        fresh.append(pool.guided_advance(*feed[t]))
    for t, (g, w) in enumerate(zip(got, fresh)):
        same(g, w, (fam, t))
    same(res, pool.guided_result(), fam)
    running = ~np.asarray(out["done"], bool)
    assert running.any() and (res[0][running].sum(1) == S2).all() and (res[2][~running] == -1).all()
    pool.guided_end()
    pool.restore(ctx.S)
    assert np.array_equal(pool.get_state(), ctx.st)


@pytest.mark.parametrize("fam", ["ConnectFour", "Hex"])
def test_sharded_pool_equals_the_unsharded(fam):
    """device=[0, 0]: two shards, the second with env_id_offset 35, one session in each; rows in request order."""
    S, results = SIMS[fam], []
    for device in ([0, 0], 0):
        env = envpool.make(f"{fam}-v1", "gymnasium", num_envs=N, device=device, seed=POOL_SEED)

        def step(act):
            if act is None:
                _, info = env.reset()
            else:
                _, _, _, _, info = env.step(act)
            return info["legal_action_mask"]

        rolled(fam, step)
        gs = env.guided_search(IDS, simulations=S, c_puct=C_PUCT, nodes=2 * S + 1)
        rec = []
        for move in range(MOVES):
            out = gs.run(lambda obs, mask, status: evaluator(obs, mask), close=False)
            assert gs.calls == S + 1
            rec.append((out, gs.reroot(out.action)))
            assert gs.calls == 0
        gs.close()
        results.append(rec)
        env.close()
    for (a, la), (b, lb) in zip(*results):
        same(a, b)
        same(la, lb)
    assert results[0][1][0].visits.sum() > results[0][0][0].visits.sum() == len(IDS) * S  # the kept visits count


def test_device_form_with_a_model_on_the_device(ctx):
    """guided_search_device(keep_open=True) and guided_reroot_device with a small seeded torch model and the played
    moves as a device tensor; the same game through the host forms, fed the numbers the model gave."""
    import torch

    from envpool_amd.torch_interop import guided_reroot_device, guided_search_device

    pool, fam, n_act, S = ctx.pool, ctx.fam, ACTIONS[ctx.fam], SIMS[ctx.fam]
    nodes = 2 * S + 1
    dev = torch.device("cuda", pool.device)
    n_obs = int(np.prod(SHAPE[fam]))
    gen = torch.Generator().manual_seed(3)
    w_p = (torch.randn((n_obs, n_act), generator=gen) * 0.3).to(dev)
    w_v = (torch.randn((n_obs,), generator=gen) * 0.2).to(dev)
    fed, seen = [], []

    def evaluate(obs, mask, status):
        assert obs.is_cuda and obs.dtype == torch.bool and mask.dtype == torch.bool and status.dtype == torch.uint8
        x = obs.reshape(obs.shape[0], -1).float()
        priors, values = torch.softmax(x @ w_p, dim=1) * mask.float(), torch.tanh(x @ w_v)
        fed.append((priors.cpu().numpy(), values.cpu().numpy()))
        seen.append((obs.cpu().numpy(), mask.cpu().numpy(), status.cpu().numpy()))
        return priors, values

    outs = [guided_search_device(pool, evaluate, IDS, S, C_PUCT, nodes=nodes, keep_open=True)]
    moves = []
    for move in range(2):
        # the played moves stay on the device; a root that is over has -1 there, which ends it (it was over already)
        actions = outs[-1][2].clone()
        if move == 1:
            actions[2] = n_act + 3  # the device form cannot look: the kernel ends that root
        moves.append(actions.cpu().numpy())
        outs.append(guided_reroot_device(pool, evaluate, actions, S))
    assert all(t.is_cuda for o in outs for t in o) and len(fed) == 3 * (S + 1)
    assert outs[2][2][2].item() == -1 and not outs[2][0][2].any()
    pool.guided_end()  # it was left open
    leaves, want = [pool.guided_begin(IDS, S, C_PUCT, nodes)], []
    for r in range(3):
        for priors, values in fed[r * (S + 1):(r + 1) * (S + 1)]:
            leaves.append(pool.guided_advance(priors, values))
        want.append(pool.guided_result())
        if r < 2:
            acts = moves[r].copy()
            ended = (acts < 0) | (acts >= n_act)
            acts[ended] = 0
            # (the host form refuses the row the kernel ended: root 2 is not compared from there on)
            leaves[-1] = pool.guided_reroot(acts, S)
    pool.guided_end()
    for r in range(3):
        rows = np.ones(len(IDS), bool)
        if r == 2:
            rows[2] = False
        same([t.cpu().numpy()[rows] for t in outs[r]], [w[rows] for w in want[r]], (fam, r))
    rows = np.ones(len(IDS), bool)
    for i, (g, w) in enumerate(zip(seen, leaves)):
        if i >= 2 * (S + 1):
            rows[2] = False
        same([x[rows] for x in g], [x[rows] for x in w], (fam, i))
    assert np.array_equal(pool.get_state(), ctx.st) and np.array_equal(pool.snapshot(), ctx.S)


def test_the_move_loop_plays_a_whole_othello_game_on_one_session():
    env = envpool.make("Othello-v1", "gymnasium", num_envs=6, seed=5)
    env.reset()
    ids = np.arange(6, dtype=np.int32)
    S = 6
    search = env.guided_search(ids, simulations=S, nodes=4 * S + 1)
    running, plies = np.ones(6, bool), 0
    while running.any():
        out = search.run(lambda obs, mask, status: stand_in(obs, mask), close=False)
        assert (out.action[running] >= 0).all() and (out.action[~running] == -1).all()
        _, _, term, trunc, info = env.step(out.action[running], ids[running])
        assert np.array_equal(info["env_id"], ids[running])
        leaves = search.reroot(np.where(running, out.action, 0))
        done = np.asarray(term, bool) | np.asarray(trunc, bool)
        assert np.array_equal(leaves[2][running] == 2, done)
        assert np.array_equal(leaves[1][running][~done], info["legal_action_mask"][~done])
        running[np.flatnonzero(running)[done]] = False
        plies += 1
        assert plies <= 130
    assert plies >= 9
    search.close()
    env.close()


def _raw_reroot(pool, actions, k, simulations):
    """epa_guided_reroot itself, past the wrapper's checks."""
    actions = np.ascontiguousarray(actions, np.int32)
    h, w, c, a = pool.guided_shape()
    n = max(k, 1)
    obs, mask, status = np.zeros((n, h, w, c), np.uint8), np.zeros((n, a), np.uint8), np.zeros(n, np.uint8)
    native.check(pool._lib.epa_guided_reroot(pool._h, actions.ctypes.data, k, simulations, obs.ctypes.data,
                                             mask.ctypes.data, status.ctypes.data))
    return obs, mask, status


def _raw_begin_nodes(pool, ids, simulations, nodes, c_puct):
    ids = np.ascontiguousarray(ids, np.int32)
    h, w, c, a = pool.guided_shape()
    k = max(len(ids), 1)
    obs, mask, status = np.zeros((k, h, w, c), np.uint8), np.zeros((k, a), np.uint8), np.zeros(k, np.uint8)
    native.check(pool._lib.epa_guided_begin_nodes(pool._h, ids.ctypes.data, len(ids), simulations, nodes,
                                                  ctypes.c_float(c_puct), obs.ctypes.data, mask.ctypes.data,
                                                  status.ctypes.data))
    return obs, mask, status


def test_refusals_and_the_session_life_cycle():
    cart = DevicePool("CartPole", 4, seed=1)
    buf = np.zeros(64, np.int32)
    with pytest.raises(RuntimeError, match="guided search not implemented"):
        native.check(cart._lib.epa_guided_reroot(cart._h, buf.ctypes.data, 2, 8, buf.ctypes.data, buf.ctypes.data,
                                                 buf.ctypes.data))
    with pytest.raises(RuntimeError, match="guided search not implemented"):
        native.check(cart._lib.epa_guided_begin_nodes(cart._h, buf.ctypes.data, 2, 8, 17, ctypes.c_float(1.0),
                                                      buf.ctypes.data, buf.ctypes.data, buf.ctypes.data))
    with pytest.raises(RuntimeError, match="guided search not implemented"):
        cart.guided_begin(None, 8, C_PUCT, 17)
    cart.close()
    ctx = get_ctx("ConnectFour")
    pool, k = ctx.pool, len(IDS)
    if getattr(pool, "_guided_k", None) is not None:
        pool.guided_end()
    acts = np.full(k, 3, np.int32)
    # without a session (never begun, or after close), through the wrapper and the C ABI
    for call in (lambda: pool.guided_reroot(acts, 8), lambda: _raw_reroot(pool, acts, k, 8)):
        with pytest.raises(ValueError, match="no guided-search session"):
            call()
    # nodes outside S + 1 .. 8192
    for nodes in (8, 8193, -1):
        with pytest.raises(ValueError, match="guided_begin: nodes"):
            pool.guided_begin(IDS, 8, C_PUCT, nodes)
        with pytest.raises(ValueError, match="guided_begin: nodes"):
            _raw_begin_nodes(pool, IDS, 8, nodes, C_PUCT)
    with pytest.raises(ValueError, match="guided_begin: nodes"):
        _raw_begin_nodes(pool, IDS, 8, 0, C_PUCT)
    with pytest.raises(ValueError, match="no guided-search session"):  # none of them opened one
        pool.guided_end()
    # on a Gumbel session
    pool.gumbel_begin(np.zeros((k, 7), F), IDS, 4)
    for call in (lambda: pool.guided_reroot(acts, 4), lambda: _raw_reroot(pool, acts, k, 4)):
        with pytest.raises(ValueError, match="gumbel|Gumbel"):
            call()
    with pytest.raises(ValueError, match="reroot not implemented for gumbel sessions"):
        _raw_reroot(pool, acts, k, 4)
    pool.guided_end()
    # before the round's last advance
    leaves = pool.guided_begin(IDS, 4, C_PUCT, 12)
    for t in range(5):
        with pytest.raises(ValueError, match="round is not complete"):
            _raw_reroot(pool, acts, k, 4)
        with pytest.raises(ValueError, match="round is not complete"):
            pool.guided_reroot(acts, 4)
        leaves = pool.guided_advance(*stand_in(leaves[0], leaves[1]))
    res = pool.guided_result()
    # rows, actions, S2 -- through the wrapper and the C ABI; none of them changes the session
    for call in (lambda: pool.guided_reroot(acts[:5], 4), lambda: _raw_reroot(pool, acts[:5], 5, 4),
                 lambda: pool.guided_reroot(np.where(np.arange(k) == 3, 7, acts), 4),
                 lambda: _raw_reroot(pool, np.where(np.arange(k) == 3, 7, acts), k, 4),
                 lambda: pool.guided_reroot(np.where(np.arange(k) == 0, -1, acts), 4),
                 lambda: _raw_reroot(pool, np.where(np.arange(k) == 0, -1, acts), k, 4),
                 lambda: pool.guided_reroot(acts, 0), lambda: _raw_reroot(pool, acts, k, 0),
                 lambda: pool.guided_reroot(acts, 4097), lambda: _raw_reroot(pool, acts, k, 4097),
                 lambda: pool.guided_reroot(acts, 12), lambda: _raw_reroot(pool, acts, k, 12)):  # S2 + 1 > C
        with pytest.raises(ValueError, match="guided_reroot"):
            call()
    same(res, pool.guided_result())
    leaves = pool.guided_reroot(acts, 11)  # S2 + 1 == C
    with pytest.raises(ValueError, match="round is not complete"):
        pool.guided_reroot(acts, 4)
    for t in range(12):
        leaves = pool.guided_advance(*stand_in(leaves[0], leaves[1]))
    with pytest.raises(ValueError, match="above simulations"):
        pool.guided_advance(*stand_in(leaves[0], leaves[1]))
    pool.guided_reroot(pool.guided_result()[2].clip(0), 4)
    pool.guided_end()
    with pytest.raises(ValueError, match="no guided-search session"):
        pool.guided_reroot(acts, 4)
    assert np.array_equal(pool.get_state(), ctx.st) and np.array_equal(pool.snapshot(), ctx.S)
    # the env classes
    env = envpool.make("TicTacToe-v1", "gymnasium", num_envs=8, seed=1)
    env.reset()
    with pytest.raises(ValueError, match="gumbel"):
        env.guided_search(simulations=4, policy="gumbel", nodes=9)
    gs = env.guided_search(simulations=4, nodes=9)
    out = gs.run(lambda obs, mask, status: stand_in(obs, mask), close=False)
    gs.reroot(out.action)
    gs.close()
    with pytest.raises(ValueError, match="closed"):
        gs.reroot(out.action)
    gs = env.guided_search(simulations=4, policy="gumbel", seed=0)
    with pytest.raises(AttributeError):
        gs.reroot  # a Gumbel session has no reroot
    env.close()
    # a pool closed with a rerooted session open
    other = DevicePool("Othello", 4, seed=1)
    other.reset(np.arange(4, dtype=np.int32))
    other.recv_dict()
    leaves = other.guided_begin(None, 3, C_PUCT, 9)
    for t in range(4):
        leaves = other.guided_advance(*stand_in(leaves[0], leaves[1]))
    other.guided_reroot(other.guided_result()[2], 3)
    other.close()


def test_trees_above_2_gib_are_refused_by_their_nodes():
    """Hex with 8192 nodes per root: the message names the most roots that fit."""
    node = 80 + 4 * 4 * 124  # (test_pgx_guided_host.py: test_node_layout)
    fits = 2**31 // (8192 * node)
    pool = DevicePool("Hex", fits + 8, seed=1)
    ids = np.arange(fits + 8, dtype=np.int32)
    pool.reset(ids)
    pool.recv_dict()
    with pytest.raises(ValueError, match=f"at most {fits} roots"):
        pool.guided_begin(ids[:fits + 1], 64, C_PUCT, 8192)
    with pytest.raises(ValueError, match=f"at most {fits} roots"):
        _raw_begin_nodes(pool, ids[:fits + 1], 64, 8192, C_PUCT)
    for nodes in (513, 600, 2049, 8192):  # the two larger tables of the reroot kernel, 8 and 32 KiB of LDS
        leaves = pool.guided_begin(ids[:3], 8, C_PUCT, nodes)
        for t in range(9):
            leaves = pool.guided_advance(*stand_in(leaves[0], leaves[1]))
        res = pool.guided_result()
        leaves = pool.guided_reroot(res[2], 8)
        assert (leaves[2] == 0).all()
        assert (pool.guided_result()[0].sum(1) == res[0][np.arange(3), res[2]] - 1).all()
    pool.close()


def teardown_module(module):
    for c in _ctx.values():
        c.pool.close()
    _ctx.clear()
