"""PGX exact solver with transposition tables (solve table_bits=) on the MI355X: the solve kernel against the host
harness of the same header with the same tables (tests/cpu_harness/pgx_solve_table_host.cpp) in all five outputs,
`nodes` included, for the four games at table_bits 0, 2 and 8 on the positions of the host test; table_bits = 0 against
the call without the keyword; rows that are given up without a table and solved with one; that no entry survives a call;
the device form, the refusals of the C entry, the other families and sharding.

The shape: a pool of 16 envs per game put at the host test's positions with set_state (one env marked over, two at the
hand-made positions), 16 ids out of order (16 blocks of one wave); ConnectFour 24 plies in with 8 roots."""
import ctypes

import numpy as np
import pytest

import envpool_amd as envpool
from envpool_amd.core import native
from envpool_amd.core.device_pool import DevicePool
from pgx_solve_table_util import (DEEP_ENVS, GIVE_BITS, GIVE_ENVS, GIVE_NODES, NAMES, build_libs, deep_connect_four,
                                  early, late_othello, table_solve)
from pgx_solve_util import BIG, DEPTHS, GAMES, hand_made, host_solve, legal_random, rolled
from pgx_util import ACTIONS

pytestmark = pytest.mark.gpu

K = 16
OVER, WIN, LOSS = 5, 9, 14  # the env marked over, the envs at the hand-made positions
IDS = np.random.default_rng(7).permutation(K).astype(np.int32)
ALL = np.arange(K, dtype=np.int32)
BITS = (0, 2, 8)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    return build_libs(tmp_path_factory.mktemp("pgx_solve_table"))


_pools = {}


def pool_of(fam):
    """The game's pool of K envs, reset once; the tests put positions in with `put`."""
    if fam not in _pools:
        _pools[fam] = pool = DevicePool(fam, K, seed=11)
        pool.reset(ALL)
        pool.recv_dict()
    return _pools[fam]


def put(pool, hid, done):
    """Envs 0 .. len(hid) - 1 at the positions; returns their rows of get_state."""
    ids = np.arange(len(hid), dtype=np.int32)
    rows = pool.get_state(ids)
    rows[:, 1], rows[:, 2:] = done, hid
    pool.set_state(rows, ids)
    return pool.get_state(ids)


def same(got, want, what, names=NAMES):
    for name, g, w in zip(names, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        assert np.array_equal(g, w), (what, name, np.flatnonzero((g != w).reshape(len(g), -1).any(1)))


def harness(libs, fam, st, depth, bits, max_nodes=BIG):
    """The harness on rows of get_state ([cur_step, done, hidden words])."""
    want, broken = table_solve(libs["solve_table_host"], fam, st[:, 2:].astype(np.int32),
                               (st[:, 1] != 0).astype(np.uint8), depth, bits, max_nodes)
    assert not broken.any()
    return want


def positions(libs, fam):
    """[(hidden [K], done [K])]: the host test's early sets cut to K rows, env OVER over, WIN and LOSS hand-made."""
    out = []
    hand = hand_made(fam)
    for hid, done in early(libs, fam):
        hid, done = hid[:K].copy(), np.zeros(K, np.uint8)
        done[OVER] = 1
        hid[WIN], hid[LOSS] = hand[0][0], hand[1][0]
        out.append((hid, done))
    return out


# ---- 8. the kernel against the harness ----------------------------------------------------------------------------
@pytest.mark.parametrize("fam", GAMES)
def test_kernel_equals_the_harness(libs, fam):
    pool = pool_of(fam)
    values = set()
    for hid, done in positions(libs, fam):
        st = put(pool, hid, done)
        for depth in DEPTHS[fam] + [3, 2]:
            plain = pool.solve(IDS, depth, BIG)
            for bits in BITS:
                got = pool.solve(IDS, depth, BIG, table_bits=bits)
                assert [g.dtype for g in got] == [np.int8, np.int8, np.int32, np.uint8, np.int64]
                assert got[1].shape == (K, ACTIONS[fam])
                same(got, harness(libs, fam, st[IDS], depth, bits), (fam, depth, bits))
                same(got[:4], plain[:4], (fam, depth, bits, "the table-less values"), NAMES[:4])
                if bits == 0:
                    same(got, plain, (fam, depth, "table_bits = 0 is the call without the keyword"))
            assert np.array_equal(plain[3], np.where(IDS == OVER, 2, 0))
            values |= set(plain[0][plain[3] == 0].tolist())
    assert values == {-1, 0, 1}  # the hand-made positions are won and lost


def test_late_othello_and_deep_connect_four(libs):
    """To the end of the game, where the tables are hit: late Othello (K roots, one over), ConnectFour 24 plies in (8
    roots)."""
    hid, done = late_othello(libs)
    hid, done = hid[:K].copy(), done[:K].copy()
    done[OVER] = 1
    deep = deep_connect_four(libs, DEEP_ENVS)
    for fam, (hid, done), ids in (("Othello", (hid, done), IDS), ("ConnectFour", deep, IDS[IDS < len(DEEP_ENVS)])):
        pool = pool_of(fam)
        st = put(pool, hid, done)
        nodes = {}
        for bits in BITS:
            got = pool.solve(ids, 0, BIG, table_bits=bits)
            same(got, harness(libs, fam, st[ids], 0, bits), (fam, bits))
            nodes[bits] = int(got[4].sum())
        same(pool.solve(ids, 0, BIG), harness(libs, fam, st[ids], 0, 0), (fam, "no keyword"))
        assert nodes[8] < nodes[2] < nodes[0], (fam, nodes)
        # a budget between the rows' sizes: the rows the harness gives up, with its `nodes`
        budget = int(np.median(pool.solve(ids, 0, BIG, table_bits=8)[4]))
        tight = pool.solve(ids, 0, budget, table_bits=8)
        same(tight, harness(libs, fam, st[ids], 0, 8, budget), (fam, "tight"))
        assert (tight[3] == 1).any() and (tight[3] == 0).any()


# ---- 9. given up becomes solved -----------------------------------------------------------------------------------
def test_given_up_without_a_table_is_solved_with_one(libs):
    hid, done = deep_connect_four(libs, GIVE_ENVS)
    pool = pool_of("ConnectFour")
    st = put(pool, hid, done)
    ids = np.arange(len(hid), dtype=np.int32)[::-1].copy()
    plain = pool.solve(ids, 0, GIVE_NODES)
    same(plain, harness(libs, "ConnectFour", st[ids], 0, 0, GIVE_NODES), "table-less")
    assert (plain[3] == 1).all() and (plain[0] == 0).all() and (plain[2] == -1).all() and (plain[1] == -128).all()
    got = pool.solve(ids, 0, GIVE_NODES, table_bits=GIVE_BITS)
    same(got, harness(libs, "ConnectFour", st[ids], 0, GIVE_BITS, GIVE_NODES), "with tables")
    want = host_solve(libs["solve_host"], "ConnectFour", hid[ids], done[ids], 0, BIG)[0]
    assert (got[3] == 0).all() and (want[3] == 0).all() and len(ids) >= 4
    same(got[:4], want[:4], "the values of the table-less harness without a budget", NAMES[:4])
    assert (want[4] > 4 * GIVE_NODES).all() and (got[4] < GIVE_NODES // 2).all()


# ---- 10. no stale entries -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["ConnectFour", "Othello"])
def test_no_entry_survives_a_call(libs, fam):
    """One pool, call after call with other depths, other orders of the roots and other positions: each call is the
    harness's (whose tables are new for every root) and a fresh pool's at the same positions.  An entry that survived
    would be found again -- the same call twice would visit fewer positions the second time."""
    pool = pool_of(fam)
    hid, done = positions(libs, fam)[0]
    put(pool, hid, done)
    fresh = DevicePool(fam, K, seed=3)
    fresh.reset(ALL)
    fresh.recv_dict()

    def check(ids, depth, what):
        st = pool.get_state()
        fresh.set_state(st, ALL)
        got = pool.solve(ids, depth, BIG, table_bits=8)
        same(got, harness(libs, fam, st[ids], depth, 8), (fam, what, "harness"))
        same(got, fresh.solve(ids, depth, BIG, table_bits=8), (fam, what, "fresh pool"))
        return got

    check(IDS, 4, "depth 4")
    first = check(IDS, 6, "depth 6")
    same(check(IDS, 6, "depth 6 again"), first, (fam, "the same call twice"))
    check(IDS[::-1].copy(), 6, "other rows")
    mask = np.stack([np.asarray(q) != -128 for q in first[1]])[np.argsort(IDS)]
    mask[OVER] = True
    pool.send(ALL, legal_random(mask, np.random.default_rng(5)))
    pool.recv_dict()
    check(IDS, 6, "one ply on")
    # to the end of the game, where the same call is sure to meet its own entries
    if fam == "Othello":
        hid, done = late_othello(libs)
        put(pool, hid[:K], done[:K])
        first = check(IDS, 0, "late")
        assert first[4].sum() < pool.solve(IDS, 0, BIG)[4].sum()
        same(check(IDS, 0, "late again"), first, "the same call twice, late")
    fresh.close()


# ---- 11. host and device forms, the C entry ------------------------------------------------------------------------
def _raw(pool, ids, depth, max_nodes, bits, n_act):
    """epa_solve_table itself, past the wrapper's checks."""
    ids = np.ascontiguousarray(ids, np.int32)
    k = max(len(ids), 1)
    value, q, action = np.zeros(k, np.int8), np.zeros((k, n_act), np.int8), np.zeros(k, np.int32)
    status, nodes = np.zeros(k, np.uint8), np.zeros(k, np.int64)
    native.check(pool._lib.epa_solve_table(pool._h, ids.ctypes.data, len(ids), depth, ctypes.c_int64(max_nodes), bits,
                                           value.ctypes.data, q.ctypes.data, action.ctypes.data, status.ctypes.data,
                                           nodes.ctypes.data))
    return value, q, action, status, nodes


def test_device_form_and_the_refusals_of_the_c_entry(libs):
    import torch

    from envpool_amd.torch_interop import solve_device

    fam = "TicTacToe"
    pool = pool_of(fam)
    hid, done = positions(libs, fam)[0]
    st = put(pool, hid, done)
    snap = pool.snapshot()
    want = harness(libs, fam, st[IDS], 0, 8)
    assert want[4].sum() < harness(libs, fam, st[IDS], 0, 0)[4].sum()
    same(pool.solve(IDS, 0, BIG, 8), want, "host form")
    dev = solve_device(pool, IDS, 0, BIG, table_bits=8)
    assert all(t.is_cuda for t in dev)
    assert [t.dtype for t in dev] == [torch.int8, torch.int8, torch.int32, torch.uint8, torch.int64]
    same([t.cpu().numpy() for t in dev], want, "device form")
    same(_raw(pool, IDS, 0, BIG, 8, 9), want, "the C entry")
    same(_raw(pool, IDS, 0, BIG, 0, 9), pool.solve(IDS, 0, BIG), "the C entry, no tables")
    for bits in (17, -1):
        with pytest.raises(ValueError, match=f"solve: table_bits = {bits} must be in 0 .. 16"):
            _raw(pool, IDS, 0, BIG, bits, 9)
    # 2^16 entries: 128 MiB of tables per root beside its stacks, so 15 roots fit under 2 GiB
    for depth, stack in ((0, 128 * 5120), (4, 4 * 5120)):
        fits = 2**31 // (64 * 32 * 2**16 + stack)
        assert fits == 15
        with pytest.raises(ValueError, match=f"tables .table_bits = 16. of 16 roots .* at most {fits} roots"):
            _raw(pool, ALL, depth, BIG, 16, 9)
        with pytest.raises(ValueError, match=f"at most {fits} roots"):
            pool.solve(ALL, depth, BIG, table_bits=16)
    # nothing was touched, and the pool solves as before
    assert np.array_equal(pool.get_state(ALL), st) and np.array_equal(pool.snapshot(), snap)
    same(pool.solve(IDS, 0, BIG, 8), want, "after the refusals")


# ---- 12. other families -------------------------------------------------------------------------------------------
def test_other_families_raise_with_the_keyword():
    from envpool_amd.torch_interop import solve_device

    cart = DevicePool("CartPole", 4, seed=1)
    with pytest.raises(RuntimeError, match="solve not implemented for this environment"):
        cart.solve(None, table_bits=4)
    with pytest.raises(RuntimeError, match="solve not implemented for this environment"):
        solve_device(cart, None, table_bits=4)
    with pytest.raises(RuntimeError, match="solve not implemented for this environment"):
        _raw(cart, [0], 0, 1, 4, 9)
    cart.close()
    env = envpool.make("CartPole-v1", "gymnasium", num_envs=4, seed=1)
    with pytest.raises(RuntimeError, match="solve not implemented for this environment"):
        env.solve(table_bits=4)
    env.close()


# ---- 13. sharding -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,plies,depth", [("TicTacToe", 2, 0), ("Othello", 3, 6)])
def test_sharded_pool_equals_the_unsharded(fam, plies, depth):
    """device=[0, 0]: two shards, the second with env_id_offset 8."""
    results = []
    for device in ([0, 0], 0):
        env = envpool.make(f"{fam}-v1", "gymnasium", num_envs=K, device=device, seed=11)

        def step(act):
            if act is None:
                _, info = env.reset()
            else:
                _, _, _, _, info = env.step(act)
            return info["legal_action_mask"]

        rolled(step, plies)
        out = env.solve(IDS, depth=depth, max_nodes=BIG, table_bits=6)
        assert out._fields == NAMES
        results.append(out)
        with pytest.raises(ValueError, match="solve: table_bits = 17 must be in 0 .. 16"):
            env.solve(IDS, table_bits=17)
        env.close()
    same(results[0], results[1], (fam, "sharded"))
    assert (results[0].status == 0).all() and (results[0].nodes > 1).all()


def teardown_module(module):
    for pool in _pools.values():
        pool.close()
    _pools.clear()
