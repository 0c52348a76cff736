"""PGX arena on the MI355X.  Kernel level: `net_eval_pair` (PgxNetPlan + the pair form of PgxNetEval), host and device
form, against the numpy net restatement (pgx_net_util.py) applied per row with the row's net, bit for bit, over rows
that do not fill a wave and every side pattern of pgx_arena_util.  Driver level: `env.arena(a, b).run(plies)` against
the same plies driven from Python -- noise rows from the self-play restatement, a session whose evaluate calls both nets
on all rows and selects by the restated side, the restated move, `env.step` -- state for state, sample for sample,
counter for counter; continuation, the enqueue-only and torch forms, sharded pools, what survives an arena, and every
refusal."""
import ctypes

import numpy as np
import pytest

import envpool_amd as envpool
import pgx_arena_util as AU
import pgx_net_util as NU
import pgx_selfplay_util as SU
from envpool_amd.core import native
from envpool_amd.core.device_pool import DevicePool
from envpool_amd.pgx.net import Net
from envpool_amd.python.envpool import ArenaStats

pytestmark = pytest.mark.gpu

SHAPE = {"TicTacToe": (3, 3, 2), "ConnectFour": (6, 7, 2), "Hex": (11, 11, 4), "Othello": (8, 8, 2)}
ACTIONS = {"TicTacToe": 9, "ConnectFour": 7, "Hex": 122, "Othello": 65}
F32 = np.float32
SENTINEL = F32(-12345.5)
# (family, (D, L) of net A, (D, L) of net B): F, A = 18, 9 and 484, 122
PAIRS = [("TicTacToe", (32, 0), (128, 2)), ("Hex", (96, 2), (32, 1))]
ROWS = [1, 63, 64, 65, 129, 257]
_pools, _made = {}, {}


def pool_of(fam):
    if fam not in _pools:
        _pools[fam] = DevicePool(fam, 4, seed=1)
    return _pools[fam]


def built(fam, d, blocks, seed):
    """(the Net, its layers, blocks and scales for the restatement)"""
    key = (fam, d, blocks, seed)
    if key not in _made:
        f, a = int(np.prod(SHAPE[fam])), ACTIONS[fam]
        layers = NU.random_layers(f, a, d, blocks, seed)
        sp, sv = NU.scales(d)
        _made[key] = (Net(SHAPE[fam], a, d, blocks, layers, sp, sv), layers, blocks, sp, sv)
    return _made[key]


def same_bits(got, want, where):
    for x, y in zip(got, want):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype == F32, where
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), where


def raw_host(pool, net_a, net_b, obs, mask, status, side, priors):
    """epa_net_eval_pair into buffers that hold a sentinel."""
    rows, a = len(status), mask.shape[1]
    policy, value = np.full((rows, a), SENTINEL, F32), np.full(rows, SENTINEL, F32)
    obs, mask, status, side = (np.ascontiguousarray(x, np.uint8) for x in (obs, mask, status, side))
    native.check(pool._lib.epa_net_eval_pair(
        pool._h, net_a._handle(pool.device), net_b._handle(pool.device), rows, int(priors), obs.ctypes.data,
        mask.ctypes.data, status.ctypes.data, side.ctypes.data, policy.ctypes.data, value.ctypes.data))
    return policy, value


def raw_device(pool, net_a, net_b, obs, mask, status, side, priors):
    """`net_eval_pair_device` on torch tensors whose outputs hold a sentinel."""
    import torch

    dev = torch.device("cuda", pool.device)
    rows, a = len(status), mask.shape[1]
    t = [torch.as_tensor(np.ascontiguousarray(x, np.uint8)).to(dev) for x in (obs, mask, status, side)]
    policy = torch.full((rows, a), float(SENTINEL), dtype=torch.float32, device=dev)
    value = torch.full((rows,), float(SENTINEL), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    pool.net_eval_pair_device(net_a, net_b, rows, priors, *(x.data_ptr() for x in t), policy.data_ptr(),
                              value.data_ptr())
    pool.synchronize()
    return policy.cpu().numpy(), value.cpu().numpy()


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: p[0])
def test_net_eval_pair_against_numpy(pair, rows):
    fam, (da, la), (db, lb) = pair
    f, a = int(np.prod(SHAPE[fam])), ACTIONS[fam]
    pool = pool_of(fam)
    net_a, *ra = built(fam, da, la, 1)
    net_b, *rb = built(fam, db, lb, 2)
    obs, mask, status = NU.random_rows(f, a, rows, seed=rows)  # statuses mix 0 (evaluate), 1 and 2 (idle)
    assert rows < 63 or {0, 1, 2} <= set(status.tolist())
    for priors in (False, True):
        per_net = [NU.restate(*r, obs, mask, status, priors) for r in (ra, rb)]  # once, shared by the patterns
        assert not np.array_equal(per_net[0][0], per_net[1][0])
        for name, side in AU.side_patterns(rows).items():
            pick = side.astype(bool)
            want = (np.where(pick[:, None], per_net[1][0], per_net[0][0]), np.where(pick, per_net[1][1], per_net[0][1]))
            for form in (raw_host, raw_device):
                got = form(pool, net_a, net_b, obs, mask, status, side, priors)
                where = (fam, rows, priors, name, form.__name__)
                assert not (got[0] == SENTINEL).any() and not (got[1] == SENTINEL).any(), where  # every row written
                assert not got[0][status != 0].any() and not got[1][status != 0].any(), where  # not to be evaluated
                same_bits(got, want, where)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: p[0])
def test_pair_of_one_net_equals_net_eval(pair):
    fam, (d, blocks), _ = pair
    f, a = int(np.prod(SHAPE[fam])), ACTIONS[fam]
    pool = pool_of(fam)
    net = built(fam, d, blocks, 1)[0]
    for rows in (65, 257):
        obs, mask, status = NU.random_rows(f, a, rows, seed=rows)
        for priors in (False, True):
            want = pool.net_eval(net, obs, mask, status, priors)
            for name in ("random", "alternating", "all1"):
                got = pool.net_eval_pair(net, net, obs, mask, status, AU.side_patterns(rows)[name], priors)
                same_bits(got, want, (fam, rows, priors, name))


# -- the arena against the host-driven loop ------------------------------------------------------------------------
_NETS = {}


def nets_of(fam):
    """Two small nets of different width and depth."""
    if fam not in _NETS:
        _NETS[fam] = (Net.random(SHAPE[fam], ACTIONS[fam], hidden=32, blocks=1, seed=1),
                      Net.random(SHAPE[fam], ACTIONS[fam], hidden=64, blocks=0, seed=2))
    return _NETS[fam]


def make(fam, n, **kw):
    return envpool.make(f"{fam}-v1", "gymnasium", num_envs=n, seed=11, **kw)


def search_kw(policy, opts):
    names = ("max_considered", "batch", "c_visit", "c_scale") if policy == "gumbel" else \
        ("c_puct", "width", "tactics", "tactics_nodes", "prove")
    return {k: v for k, v in opts.items() if k in names}


class Run:
    def __init__(self, samples, counters, state, stats):
        self.samples, self.counters, self.state, self.stats = samples, counters, state, stats


def same_samples(a, b, what=""):
    assert a._fields == b._fields
    for name, x, y in zip(a._fields, a, b):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, name, x.shape, y.shape)
        assert x.tobytes() == y.tobytes(), (what, name)


def same_runs(a, b, what=""):
    if a.samples is not None:
        same_samples(a.samples, b.samples, what)
        assert a.counters == b.counters, what
    if a.state is not None:
        assert a.state.tobytes() == b.state.tobytes(), what
    assert tuple(a.stats) == tuple(b.stats), (what, a.stats, b.stats)


def state_of(env):
    pool = env.device_pool
    return pool.get_state() if hasattr(pool, "get_state") else None


def split(kw):
    env_kw = {k: v for k, v in kw.items() if k in ("env_id_offset", "device")}
    return env_kw, {k: v for k, v in kw.items() if k not in env_kw}


def arena_run(fam, n, plies, policy, seed=5, record=True, parts=None, nets=None, close_env=True, wait=True, **kw):
    """Pool A: the arena.  `parts`: the plies as several run calls."""
    env_kw, opts = split(kw)
    env = make(fam, n, **env_kw)
    rec = env.recorder(capacity=1 << 15) if record else None
    env.reset()
    a, b = nets or nets_of(fam)
    arena = env.arena(a, b, policy=policy, simulations=8, seed=seed, record=record, **opts)
    for p in parts or [plies]:
        stats = arena.run(p, wait=wait)
    if not wait:
        assert stats is None
        stats = arena.stats()
    out = Run(rec.drain() if record else None, rec.counters if record else None, state_of(env), stats)
    if not close_env:
        return out, env, rec, arena
    arena.close()
    env.close()
    return out


def host_run(fam, n, plies, policy, seed=5, record=True, close_env=True, **kw):
    """Pool B: the match driven from Python, ply by ply, with both nets on all rows."""
    env_kw, opts = split(kw)
    env = make(fam, n, **env_kw)
    a = ACTIONS[fam]
    net_a, net_b = nets_of(fam)
    priors = policy == "puct"
    both = [net.bind(env, priors) for net in (net_a, net_b)]
    rec = env.recorder(capacity=1 << 15) if record else None
    _, info = env.reset()
    ids = np.asarray(env.all_env_ids)
    elapsed = np.asarray(info["elapsed_step"]).reshape(-1)
    total = np.zeros(7, np.int64)
    for t in range(plies):
        side = AU.net_of(ids, np.asarray(info["current_player"]).reshape(-1))  # fixed for the ply

        def evaluate(obs, mask, status):
            (pa, va), (pb, vb) = (ev(obs, mask, status) for ev in both)
            rows = pa.reshape(-1, a).shape[0]
            s = np.repeat(side, rows // n).astype(bool)
            return (np.where(s[:, None], pb.reshape(-1, a), pa.reshape(-1, a)).reshape(pa.shape),
                    np.where(s, vb.reshape(-1), va.reshape(-1)).reshape(va.shape))

        if policy == "gumbel":
            noise = SU.noise_rows(seed, ids, t, a, opts.get("noise", True))
            result = env.gumbel_search(simulations=8, gumbel=noise, **search_kw(policy, opts)).run(evaluate)
            action, target = SU.gumbel_move(result.action, result.weights)
        else:
            result = env.guided_search(simulations=8, **search_kw(policy, opts)).run(evaluate)
            action, target = SU.puct_move(result.visits, result.action, elapsed, opts.get("sample_plies", 0),
                                          SU.key(seed, ids, t))
        if record:
            rec.add(target)
        _, rew, term, trunc, info = env.step(action)
        if record:
            rec.finish(rew, term | trunc)
        elapsed = np.asarray(info["elapsed_step"]).reshape(-1)
        total += AU.tally(term | trunc, rew, elapsed, ids)
    stats = ArenaStats(*(int(x) for x in total), plies)
    out = Run(rec.drain() if record else None, rec.counters if record else None, state_of(env), stats)
    if not close_env:
        return out, env, rec
    env.close()
    return out


CONFIGS = [
    ("TicTacToe", 48, 12, "gumbel", dict(max_considered=4)),
    ("TicTacToe", 48, 12, "gumbel", dict(max_considered=4, batch=4)),
    ("ConnectFour", 48, 8, "puct", dict(sample_plies=4, width=2)),
    ("Othello", 24, 6, "gumbel", dict(max_considered=4)),
    ("Hex", 24, 4, "gumbel", dict(max_considered=4)),  # (the mover comes from HexCurrent)
]


@pytest.mark.parametrize("fam,n,plies,policy,opts", CONFIGS, ids=lambda x: str(x).replace(" ", ""))
def test_arena_equals_the_host_driven_loop(fam, n, plies, policy, opts):
    got, env_a, rec_a, arena = arena_run(fam, n, plies, policy, close_env=False, **opts)
    want, env_b, rec_b = host_run(fam, n, plies, policy, close_env=False, **opts)
    same_runs(got, want, (fam, policy, opts))
    s = got.stats
    assert isinstance(s, ArenaStats) and s.t == plies
    assert s.wins_a + s.wins_b + s.draws == s.games and s.wins0 + s.wins1 == s.wins_a + s.wins_b
    if fam == "TicTacToe":
        assert s.games >= n and got.counters["games"] == s.games  # every env finished a game and began another
    # the two nets do play differently: an arena of (a, a) leaves other states
    if fam == "TicTacToe" and "batch" not in opts:
        one = arena_run(fam, n, plies, policy, nets=(nets_of(fam)[0],) * 2, **opts)
        assert one.state.tobytes() != got.state.tobytes()
    # selfplay after an arena, and a plain search after it, on both pools alike
    assert tuple(env_a.device_pool.selfplay_stats()) == tuple(s[:5]) + (s.t,)  # the six values of an arena
    arena.close()
    with pytest.raises(ValueError, match="arena: the arena is closed"):
        arena.stats()
    net = nets_of(fam)[0]
    sp_a = env_a.selfplay(net, policy=policy, simulations=8, seed=9, record=False, **opts)
    sp_b = env_b.selfplay(net, policy=policy, simulations=8, seed=9, record=False, **opts)
    assert tuple(sp_a.run(2)) == tuple(sp_b.run(2))
    with pytest.raises(ValueError, match="arena_stats: the pool has no arena"):
        env_a.device_pool.arena_stats()
    sp_a.close()
    sp_b.close()
    assert state_of(env_a).tobytes() == state_of(env_b).tobytes()
    zeros = np.zeros((n, ACTIONS[fam]), np.float32)
    after = [env.gumbel_search(simulations=8, max_considered=4, gumbel=zeros).run(net) for env in (env_a, env_b)]
    for x, y in zip(*after):
        assert x.tobytes() == y.tobytes()
    env_a.close()
    env_b.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_pool_sizes_with_an_odd_offset(n):
    """An odd offset flips every side; pools that do not fill a wave of any of the kernels."""
    got = arena_run("TicTacToe", n, 10, "gumbel", env_id_offset=3, max_considered=4)
    want = host_run("TicTacToe", n, 10, "gumbel", env_id_offset=3, max_considered=4)
    same_runs(got, want, n)
    assert got.stats.games >= n
    if n >= 63:
        flipped = arena_run("TicTacToe", n, 10, "gumbel", env_id_offset=4, max_considered=4, record=False)
        assert flipped.state.tobytes() != got.state.tobytes()


def test_arena_of_one_net_is_selfplay():
    fam, n = "TicTacToe", 48
    net = nets_of(fam)[0]
    got = arena_run(fam, n, 12, "gumbel", nets=(net, net), max_considered=4, batch=4)
    env = make(fam, n)
    rec = env.recorder(capacity=1 << 15)
    env.reset()
    sp = env.selfplay(net, policy="gumbel", simulations=8, seed=5, max_considered=4, batch=4)
    stats = sp.run(12)
    same_samples(got.samples, rec.drain())
    assert got.state.tobytes() == state_of(env).tobytes()
    assert tuple(got.stats[:5]) == tuple(stats[:5]) and got.stats.t == stats.t
    assert got.stats.wins_a + got.stats.wins_b + got.stats.draws == got.stats.games
    sp.close()
    env.close()


def test_continuation_and_enqueue_only():
    whole = arena_run("ConnectFour", 40, 5, "gumbel", max_considered=4)
    same_runs(arena_run("ConnectFour", 40, 5, "gumbel", max_considered=4, parts=[3, 2]), whole)
    same_runs(arena_run("ConnectFour", 40, 5, "gumbel", max_considered=4, parts=[4, 1], wait=False), whole)
    assert whole.stats.t == 5


def test_torch_form_equals_the_host_form():
    import torch

    from envpool_amd.torch_interop import arena_device

    fam = "Othello"
    want = arena_run(fam, 24, 5, "puct", sample_plies=2, width=2)
    env = make(fam, 24)
    pool = env.device_pool
    rec = env.recorder(capacity=1 << 15)
    env.reset()
    a, b = nets_of(fam)
    dev = torch.device("cuda", pool.device)
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        arena_device(pool, a, b, 3, policy="puct", simulations=8, seed=5, sample_plies=2, width=2, record=True)
        arena_device(pool, a, b, 2)  # the open arena continues
        torch.cuda.current_stream(dev).synchronize()
    stats = ArenaStats(*(int(x) for x in pool.arena_stats()))
    same_runs(Run(rec.drain(), rec.counters, state_of(env), stats), want)
    pool.arena_end()
    env.close()


def same_per_env(one, two, n):
    assert tuple(one.stats) == tuple(two.stats) and one.counters == two.counters
    for e in range(n):
        for name, x, y in zip(one.samples._fields, one.samples, two.samples):
            assert x[one.samples.env_id == e].tobytes() == y[two.samples.env_id == e].tobytes(), (e, name)


def test_sharded_pool_plays_the_unsharded_pools_match():
    """34 envs in two shards: the second shard's first env has the odd global id 17 and the local id 0."""
    one = arena_run("TicTacToe", 34, 12, "gumbel", max_considered=4, batch=4)
    two = arena_run("TicTacToe", 34, 12, "gumbel", max_considered=4, batch=4, device=[0, 0])
    same_per_env(one, two, 34)


def test_two_shards_on_one_device_enqueue_only():
    n, fam = 64, "TicTacToe"
    one = arena_run(fam, n, 12, "gumbel", max_considered=4)
    two = arena_run(fam, n, 12, "gumbel", max_considered=4, device=[0, 0], parts=[5, 4, 3], wait=False)
    same_per_env(one, two, n)
    assert two.stats.games >= n


def test_refusals():
    fam = "TicTacToe"
    a, b = nets_of(fam)
    other = nets_of("ConnectFour")[0]
    env = make(fam, 8)
    pool = env.device_pool
    with pytest.raises(ValueError, match="arena: net_b must be an envpool_amd.pgx.net.Net"):
        env.arena(a, lambda *x: None)
    with pytest.raises(ValueError, match="arena: net_a has F = 18, A = 9 and net_b F = 84, A = 7"):
        env.arena(a, other)
    with pytest.raises(ValueError, match="arena: net_a has F = 84, A = 7 and net_b F = 18, A = 9"):
        env.evaluate_pair(other, a, np.zeros(8, np.uint8))
    with pytest.raises(ValueError, match="arena_begin: a net of F = 84, A = 7 for a pool of F = 18, A = 9"):
        env.arena(other, other)
    with pytest.raises(ValueError, match="arena_stats: the pool has no arena"):
        pool.arena_stats()
    with pytest.raises(ValueError, match="arena_begin: record needs an open recorder"):
        env.arena(a, b, record=True)
    with pytest.raises(ValueError, match=r"selfplay: \['width'\] are arguments of policy='puct'"):
        env.arena(a, b, width=2)
    pool.reset(np.arange(8, dtype=np.int32))
    with pytest.raises(ValueError, match="arena_begin: 8 rows are pending in the pool's result queue"):
        env.arena(a, b)
    pool.recv()
    ha, hb = a._handle(pool.device), b._handle(pool.device)
    o = native.check_arena(a, b)

    def raw(**kw):
        o = native.check_selfplay(record=False, **{k: v for k, v in kw.items() if k == "policy"})
        for k, v in kw.items():
            if k != "policy":
                setattr(o, k, v)
        return pool._lib.epa_arena_begin(pool._h, ha, hb, ctypes.byref(o))

    for kw, msg in [
        (dict(simulations=0), "gumbel_begin: simulations = 0 must be 1 .. 4096"),
        (dict(batch=33), "gumbel_begin: batch = 33 must be 1 .. 32"),
        (dict(width=2), "arena_begin: width is an argument of the PUCT policy"),
        (dict(sample_plies=2), "arena_begin: sample_plies is an argument of the PUCT policy"),
        (dict(policy="puct", noise=1), "arena_begin: noise is an argument of the Gumbel policy"),
        (dict(policy="puct", batch=4), "arena_begin: batch is an argument of the Gumbel policy"),
        (dict(policy="puct", width=33), "guided_begin: width = 33 must be 1 .. 32"),
        (dict(policy="puct", sample_plies=-1), "arena_begin: sample_plies = -1 must be >= 0"),
        (dict(record=1), "arena_begin: record needs an open recorder"),
        (dict(noise=2), "arena_begin: noise and record must be 0 or 1"),
    ]:
        with pytest.raises(ValueError, match=msg):
            native.check(raw(**kw))
    o.policy = 2
    with pytest.raises(ValueError, match="arena_begin: policy = 2 must be"):
        native.check(pool._lib.epa_arena_begin(pool._h, ha, hb, ctypes.byref(o)))
    o = native.check_arena(a, b)
    for x, y in ((None, hb), (ha, None)):
        with pytest.raises(ValueError, match="arena_begin: null argument"):
            native.check(pool._lib.epa_arena_begin(pool._h, x, y, ctypes.byref(o)))
    with pytest.raises(ValueError, match="arena_begin: a net of F = 84, A = 7 for a pool of F = 18, A = 9"):
        native.check(pool._lib.epa_arena_begin(pool._h, ha, other._handle(pool.device), ctypes.byref(o)))
    if native.device_count() > 1:
        with pytest.raises(ValueError, match="arena_begin: the net is on device 1, the pool on device 0"):
            native.check(pool._lib.epa_arena_begin(pool._h, ha, b._handle(1), ctypes.byref(o)))
    # the direct form
    obs, mask, status = NU.random_rows(18, 9, 5, seed=1)
    side = np.array([0, 1, 0, 1, 1], np.uint8)
    with pytest.raises(ValueError, match="net_eval_pair: side must be 0 .net_a. or 1 .net_b. in every row"):
        pool.net_eval_pair(a, b, obs, mask, status, [0, 1, 2, 0, 0])
    with pytest.raises(ValueError, match=r"net_eval_pair: side has shape \(4,\) for 5 rows"):
        pool.net_eval_pair(a, b, obs, mask, status, side[:4])
    bad = np.array([0, 1, 0, 7, 1], np.uint8)
    with pytest.raises(ValueError, match=r"net_eval_pair: side\[3\] = 7 must be 0 \(net_a\) or 1 \(net_b\)"):
        raw_host(pool, a, b, obs, mask, status, bad, False)
    with pytest.raises(ValueError, match="net_eval_pair: a net of F = 84, A = 7 for a pool of F = 18, A = 9"):
        raw_host(pool, a, other, obs, mask, status, side, False)
    with pytest.raises(ValueError, match="net_eval_pair: rows = 0 must be 1 .. 1048576"):
        native.check(pool._lib.epa_net_eval_pair(pool._h, ha, hb, 0, 0, obs.ctypes.data, mask.ctypes.data,
                                                 status.ctypes.data, side.ctypes.data, obs.ctypes.data,
                                                 obs.ctypes.data))
    with pytest.raises(ValueError, match="net_eval_pair: mode = 2 must be 0 .logits. or 1 .priors."):
        native.check(pool._lib.epa_net_eval_pair(pool._h, ha, hb, 5, 2, obs.ctypes.data, mask.ctypes.data,
                                                 status.ctypes.data, side.ctypes.data, obs.ctypes.data,
                                                 obs.ctypes.data))
    with pytest.raises(ValueError, match="net_eval_pair: null argument"):
        native.check(pool._lib.epa_net_eval_pair(pool._h, ha, hb, 5, 0, obs.ctypes.data, mask.ctypes.data,
                                                 status.ctypes.data, None, obs.ctypes.data, obs.ctypes.data))
    # evaluate_pair works after all that, and equals evaluate row by row
    env.reset()
    got = env.evaluate_pair(a, b, [0, 1, 1, 0, 0, 1, 0, 1])
    ea, eb = env.evaluate(a), env.evaluate(b)
    pick = np.array([0, 1, 1, 0, 0, 1, 0, 1], bool)
    same_bits(got, (np.where(pick[:, None], eb[0], ea[0]), np.where(pick, eb[1], ea[1])), "evaluate_pair")
    env.close()
    # async mode
    env = make(fam, 8, batch_size=4)
    with pytest.raises(ValueError, match="arena: async mode"):
        env.arena(a, b)
    with pytest.raises(ValueError, match=r"arena_begin: async mode \(batch_size = 4 of num_envs = 8\)"):
        env.device_pool.arena_begin(a, b)
    env.close()
    # a family without guided search
    env = envpool.make("CartPole-v1", "gymnasium", num_envs=2, seed=1)
    with pytest.raises(RuntimeError, match="guided search not implemented for this environment"):
        env.arena(a, b)
    env.close()
