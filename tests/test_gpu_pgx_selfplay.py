"""PGX self-play driver on the MI355X: `env.selfplay(net, ...).run(plies)` against the same plies driven from Python
-- noise rows from the numpy restatement (pgx_selfplay_util), `search.run(net)`, `rec.add`, `env.step`, `rec.finish` --
sample for sample, byte for byte; the lane-mapping edges; continuation across run calls; the enqueue-only and torch
forms; a sharded pool; what survives the driver; every refusal."""
import ctypes

import numpy as np
import pytest

import envpool_amd as envpool
import pgx_selfplay_util as U
from envpool_amd.core import native
from envpool_amd.pgx.net import Net

pytestmark = pytest.mark.gpu

SHAPE = {"TicTacToe": (3, 3, 2), "ConnectFour": (6, 7, 2), "Hex": (11, 11, 4), "Othello": (8, 8, 2)}
ACTIONS = {"TicTacToe": 9, "ConnectFour": 7, "Hex": 122, "Othello": 65}
_NETS = {}


def net_of(fam):
    """A small net throughout: hidden 32, one block."""
    if fam not in _NETS:
        _NETS[fam] = Net.random(SHAPE[fam], ACTIONS[fam], hidden=32, blocks=1, seed=1)
    return _NETS[fam]


def make(fam, n, **kw):
    return envpool.make(f"{fam}-v1", "gymnasium", num_envs=n, seed=11, **kw)


def search_kw(policy, opts):
    """The options of `selfplay` that the searches of the host-driven loop take."""
    names = ("max_considered", "batch", "c_visit", "c_scale") if policy == "gumbel" else \
        ("c_puct", "width", "tactics", "tactics_nodes", "prove")
    return {k: v for k, v in opts.items() if k in names}


class Run:
    """What a run leaves: the drained samples, the recorder's counters, the envs' states, the statistics."""

    def __init__(self, samples, counters, state, stats):
        self.samples, self.counters, self.state, self.stats = samples, counters, state, stats


def same_samples(a, b, what=""):
    assert a._fields == b._fields
    for name, x, y in zip(a._fields, a, b):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, name, x.shape, y.shape)
        assert x.tobytes() == y.tobytes(), (what, name)


def same_runs(a, b, what=""):
    same_samples(a.samples, b.samples, what)
    assert a.counters == b.counters, what
    if a.state is not None:
        assert np.array_equal(a.state, b.state), what
    assert tuple(a.stats) == tuple(b.stats), (what, a.stats, b.stats)


def state_of(env):
    pool = env.device_pool
    return pool.get_state() if hasattr(pool, "get_state") else None


def driver_run(fam, n, plies, policy, seed=5, symmetries=False, parts=None, close_env=True, **kw):
    """Pool A: the driver.  `parts`: the plies as several run calls."""
    opts = {k: v for k, v in kw.items() if k not in ("env_id_offset", "device")}
    env = make(fam, n, **{k: v for k, v in kw.items() if k in ("env_id_offset", "device")})
    rec = env.recorder(capacity=1 << 15, symmetries=symmetries)
    env.reset()
    sp = env.selfplay(net_of(fam), policy=policy, simulations=8, seed=seed, **opts)
    for p in parts or [plies]:
        stats = sp.run(p)
    out = Run(rec.drain(), rec.counters, state_of(env), stats)
    if not close_env:
        return out, env, rec, sp
    sp.close()
    rec.close()
    env.close()
    return out


def host_run(fam, n, plies, policy, seed=5, symmetries=False, close_env=True, **kw):
    """Pool B: the README's loop in Python, with the restatement's noise and move rules."""
    opts = {k: v for k, v in kw.items() if k not in ("env_id_offset", "device")}
    env = make(fam, n, **{k: v for k, v in kw.items() if k in ("env_id_offset", "device")})
    net, a = net_of(fam), ACTIONS[fam]
    rec = env.recorder(capacity=1 << 15, symmetries=symmetries)
    _, info = env.reset()
    ids = env.all_env_ids
    elapsed = np.asarray(info["elapsed_step"]).reshape(-1)
    total = np.zeros(5, np.int64)
    for t in range(plies):
        if policy == "gumbel":
            noise = U.noise_rows(seed, ids, t, a, opts.get("noise", True))
            result = env.gumbel_search(simulations=8, gumbel=noise, **search_kw(policy, opts)).run(net)
            action, target = U.gumbel_move(result.action, result.weights)
        else:
            result = env.guided_search(simulations=8, **search_kw(policy, opts)).run(net)
            action, target = U.puct_move(result.visits, result.action, elapsed, opts.get("sample_plies", 0),
                                         U.key(seed, ids, t))
        rec.add(target)
        _, rew, term, trunc, info = env.step(action)
        rec.finish(rew, term | trunc)
        elapsed = np.asarray(info["elapsed_step"]).reshape(-1)
        total += U.tally(term | trunc, rew, elapsed)
    out = Run(rec.drain(), rec.counters, state_of(env), tuple(int(x) for x in total) + (plies,))
    if not close_env:
        return out, env, rec
    rec.close()
    env.close()
    return out


def second_games(samples):
    """Envs with a sample of ply 0 that belongs to a later game than the env's first."""
    first = (samples.ply == 0) & (samples.sym == 0)
    ids, counts = np.unique(samples.env_id[first], return_counts=True)
    return ids[counts > 1]


CONFIGS = [
    ("TicTacToe", 48, 12, "gumbel", dict(max_considered=4), True),
    ("TicTacToe", 48, 12, "gumbel", dict(max_considered=4, batch=4), True),
    ("Othello", 24, 6, "gumbel", dict(max_considered=4), False),
    ("Hex", 24, 4, "gumbel", dict(max_considered=4), False),
    ("TicTacToe", 48, 12, "puct", dict(sample_plies=4, width=2), True),
    ("ConnectFour", 48, 12, "puct", dict(sample_plies=4, width=2), True),
    # two actions per lane of the PUCT move's lane group (A = 65 and 122): sampled and greedy plies
    ("Othello", 24, 6, "puct", dict(sample_plies=4), False),
    ("Hex", 24, 4, "puct", dict(sample_plies=2, width=2), False),
]


@pytest.mark.parametrize("fam,n,plies,policy,opts,sym", CONFIGS, ids=lambda x: str(x).replace(" ", ""))
def test_driver_equals_the_host_driven_loop(fam, n, plies, policy, opts, sym):
    got, env_a, rec_a, sp = driver_run(fam, n, plies, policy, symmetries=sym, close_env=False, **opts)
    want, env_b, rec_b = host_run(fam, n, plies, policy, symmetries=sym, close_env=False, **opts)
    same_runs(got, want, (fam, policy, opts))
    assert got.stats.t == plies and len(got.samples.ply) == got.counters["samples"]
    if fam == "TicTacToe":
        # a game lasts at most 9 plies and a reset takes one: every env finishes a game, and some env begins a second
        # one whose first ply is a sample -- the reset path was exercised
        assert got.stats.games >= n and got.counters["games"] == got.stats.games
        assert got.stats.wins0 + got.stats.wins1 + got.stats.draws == got.stats.games
        assert len(second_games(got.samples)) > 0
    if policy == "puct":
        assert np.allclose(got.samples.policy.sum(axis=1), 1.0, atol=1e-5)
    # an open recorder survives the driver's close, and a plain search after a driver works
    sp.close()
    assert rec_a.counters == got.counters
    zeros = np.zeros((n, ACTIONS[fam]), np.float32)
    after_a = env_a.gumbel_search(simulations=8, max_considered=4, gumbel=zeros).run(net_of(fam))
    after_b = env_b.gumbel_search(simulations=8, max_considered=4, gumbel=zeros).run(net_of(fam))
    for x, y in zip(after_a, after_b):
        assert x.tobytes() == y.tobytes()
    # ... and so does a step through the host path: the driver's batches are out of the result queue
    played = [env.step(np.where(after_a.action < 0, 0, after_a.action)) for env in (env_a, env_b)]
    for x, y in zip(played[0][:4], played[1][:4]):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    with pytest.raises(ValueError, match="selfplay: the driver is closed"):
        sp.stats()
    for rec, env in ((rec_a, env_a), (rec_b, env_b)):
        rec.close()
        env.close()


@pytest.mark.parametrize("policy,opts", [("gumbel", dict(max_considered=4)), ("puct", dict(sample_plies=3))], ids=str)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_lane_mapping_edges(n, policy, opts):
    got = driver_run("TicTacToe", n, 10, policy, env_id_offset=3, **opts)
    want = host_run("TicTacToe", n, 10, policy, env_id_offset=3, **opts)
    same_runs(got, want, (n, policy))
    assert got.stats.games >= n
    assert got.samples.env_id.min() >= 3 and got.samples.env_id.max() < 3 + n


def test_continuation_noise_and_seeds():
    whole = driver_run("TicTacToe", 32, 5, "gumbel", max_considered=4)
    parts = driver_run("TicTacToe", 32, 5, "gumbel", max_considered=4, parts=[3, 2])
    same_runs(whole, parts)
    assert parts.stats.t == 5
    quiet = [driver_run("TicTacToe", 32, 8, "gumbel", max_considered=4, noise=False, seed=s) for s in (1, 2)]
    same_runs(quiet[0], quiet[1])  # without noise the seed does not matter
    loud = [driver_run("TicTacToe", 32, 8, "gumbel", max_considered=4, seed=s) for s in (1, 2)]
    assert loud[0].samples.policy.tobytes() != loud[1].samples.policy.tobytes()
    sampled = [driver_run("TicTacToe", 32, 8, "puct", sample_plies=9, seed=s) for s in (1, 2)]
    assert not np.array_equal(sampled[0].state, sampled[1].state)


def test_enqueue_only_then_stats():
    want = driver_run("ConnectFour", 40, 6, "gumbel", max_considered=4)
    env = make("ConnectFour", 40)
    rec = env.recorder(capacity=1 << 15)
    env.reset()
    sp = env.selfplay(net_of("ConnectFour"), simulations=8, seed=5, max_considered=4)
    assert sp.run(4, wait=False) is None
    assert sp.run(2, wait=False) is None
    stats = sp.stats()
    same_runs(Run(rec.drain(), rec.counters, state_of(env), stats), want)
    sp.close()
    env.close()


def test_torch_form_equals_the_host_form():
    import torch

    from envpool_amd.torch_interop import selfplay_device

    fam = "Othello"
    want = driver_run(fam, 24, 5, "puct", sample_plies=2, width=2)
    env = make(fam, 24)
    pool = env.device_pool
    rec = env.recorder(capacity=1 << 15)
    env.reset()
    dev = torch.device("cuda", pool.device)
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        selfplay_device(pool, net_of(fam), 3, policy="puct", simulations=8, seed=5, sample_plies=2, width=2)
        selfplay_device(pool, net_of(fam), 2)  # the open driver continues
        torch.cuda.current_stream(dev).synchronize()
    stats = pool.selfplay_stats()
    same_runs(Run(rec.drain(), rec.counters, state_of(env), tuple(int(x) for x in stats)), want)
    pool.selfplay_end()
    env.close()


def same_per_env(one, two, n):
    assert tuple(one.stats) == tuple(two.stats) and one.counters == two.counters
    # the shards' samples come shard by shard: the same samples, env by env in the same order
    for e in range(n):
        for name, x, y in zip(one.samples._fields, one.samples, two.samples):
            assert x[one.samples.env_id == e].tobytes() == y[two.samples.env_id == e].tobytes(), (e, name)


def test_sharded_pool_plays_the_unsharded_pools_games():
    one = driver_run("TicTacToe", 32, 12, "gumbel", max_considered=4, batch=4)
    two = driver_run("TicTacToe", 32, 12, "gumbel", max_considered=4, batch=4, device=[0, 0])
    same_per_env(one, two, 32)


def test_sharded_pool_enqueue_only_plain_session():
    """Two shards on one device share the net's copy and its policy and value rows: `wait=False` must not let their
    rounds overlap on the device.  A plain session (no host wait inside a round), several run calls."""
    n, fam = 64, "TicTacToe"
    one = driver_run(fam, n, 12, "gumbel", max_considered=4)
    env = make(fam, n, device=[0, 0])
    rec = env.recorder(capacity=1 << 15)
    env.reset()
    sp = env.selfplay(net_of(fam), simulations=8, seed=5, max_considered=4)
    for plies in (5, 4, 3):
        assert sp.run(plies, wait=False) is None
    two = Run(rec.drain(), rec.counters, None, sp.stats())
    sp.close()
    rec.close()
    env.close()
    same_per_env(one, two, n)
    assert two.stats.games >= n


def test_refusals():
    fam = "TicTacToe"
    net, other = net_of(fam), net_of("ConnectFour")
    env = make(fam, 8)
    pool = env.device_pool
    with pytest.raises(ValueError, match="selfplay: net must be an envpool_amd.pgx.net.Net"):
        env.selfplay(lambda *a: None)
    with pytest.raises(ValueError, match="selfplay_run: the pool has no self-play driver"):
        pool.selfplay_run(1)
    with pytest.raises(ValueError, match="selfplay_stats: the pool has no self-play driver"):
        pool.selfplay_stats()
    with pytest.raises(ValueError, match="selfplay_end: the pool has no self-play driver"):
        pool.selfplay_end()
    with pytest.raises(ValueError, match="selfplay_begin: a net of F = 84, A = 7 for a pool of F = 18, A = 9"):
        env.selfplay(other, record=False)
    with pytest.raises(ValueError, match="selfplay_begin: record needs an open recorder"):
        env.selfplay(net)
    with pytest.raises(ValueError, match=r"selfplay: \['width'\] are arguments of policy='puct'"):
        env.selfplay(net, width=2)
    # rows pending in the result queue
    pool.reset(np.arange(8, dtype=np.int32))
    with pytest.raises(ValueError, match="selfplay_begin: 8 rows are pending in the pool's result queue"):
        env.selfplay(net, record=False)
    pool.recv()
    sp = env.selfplay(net, record=False, simulations=4)
    with pytest.raises(ValueError, match="selfplay_run: plies = 0 must be at least 1"):
        sp.run(0)
    with pytest.raises(ValueError, match="selfplay_run: plies = -1 must be at least 1"):
        native.check(pool._lib.epa_selfplay_run(pool._h, -1))
    pool.reset(np.arange(8, dtype=np.int32))
    with pytest.raises(ValueError, match="selfplay_run: 8 rows are pending"):
        sp.run(1)
    pool.recv()
    assert sp.run(2).t == 2
    sp.close()
    # the engine's own refusals, through the raw call: what the Python checks would have stopped
    h = net._handle(pool.device)

    def raw(**kw):
        o = native.check_selfplay(record=False, **{k: v for k, v in kw.items() if k == "policy"})
        for k, v in kw.items():
            if k != "policy":
                setattr(o, k, v)
        return pool._lib.epa_selfplay_begin(pool._h, h, ctypes.byref(o))

    for kw, msg in [
        (dict(simulations=0), "gumbel_begin: simulations = 0 must be 1 .. 4096"),
        (dict(max_considered=0), "gumbel_begin: max_considered = 0 must be at least 1"),
        (dict(batch=33), "gumbel_begin: batch = 33 must be 1 .. 32"),
        (dict(c_visit=-1.0), "gumbel_begin: c_visit and c_scale must be finite and >= 0"),
        (dict(width=2), "selfplay_begin: width is an argument of the PUCT policy"),
        (dict(sample_plies=2), "selfplay_begin: sample_plies is an argument of the PUCT policy"),
        (dict(prove=1), "selfplay_begin: prove is an argument of the PUCT policy"),
        (dict(c_puct=1.25), "selfplay_begin: c_puct is an argument of the PUCT policy"),
        (dict(tactics_nodes=4096), "selfplay_begin: tactics_nodes is an argument of the PUCT policy"),
        (dict(policy="puct", noise=1), "selfplay_begin: noise is an argument of the Gumbel policy"),
        (dict(policy="puct", c_visit=50.0), "selfplay_begin: c_visit is an argument of the Gumbel policy"),
        (dict(policy="puct", c_scale=0.1), "selfplay_begin: c_scale is an argument of the Gumbel policy"),
        (dict(policy="puct", max_considered=4), "selfplay_begin: max_considered is an argument of the Gumbel policy"),
        (dict(policy="puct", batch=4), "selfplay_begin: batch is an argument of the Gumbel policy"),
        (dict(policy="puct", simulations=5000), "guided_begin: simulations = 5000 must be 1 .. 4096"),
        (dict(policy="puct", width=33), "guided_begin: width = 33 must be 1 .. 32"),
        (dict(policy="puct", tactics=17), "guided_begin: tactics = 17 must be 0 .. 16"),
        (dict(policy="puct", c_puct=-1.0), "guided_begin: c_puct must be finite and >= 0"),
        (dict(policy="puct", sample_plies=-1), "selfplay_begin: sample_plies = -1 must be >= 0"),
        (dict(record=1), "selfplay_begin: record needs an open recorder"),
        (dict(noise=2), "selfplay_begin: noise and record must be 0 or 1"),
    ]:
        with pytest.raises(ValueError, match=msg):
            native.check(raw(**kw))
    o = native.check_selfplay(record=False)
    o.policy = 2
    with pytest.raises(ValueError, match="selfplay_begin: policy = 2 must be"):
        native.check(pool._lib.epa_selfplay_begin(pool._h, h, ctypes.byref(o)))
    with pytest.raises(ValueError, match="selfplay_begin: null argument"):
        native.check(pool._lib.epa_selfplay_begin(pool._h, None, ctypes.byref(o)))
    if native.device_count() > 1:
        with pytest.raises(ValueError, match="selfplay_begin: the net is on device 1, the pool on device 0"):
            native.check(pool._lib.epa_selfplay_begin(pool._h, net._handle(1), ctypes.byref(o)))
    # a recorder that was closed under a recording driver
    rec = env.recorder(capacity=64)
    sp = env.selfplay(net, simulations=4)
    rec.close()
    with pytest.raises(ValueError, match="selfplay_run: record needs an open recorder"):
        sp.run(1)
    sp.close()
    env.close()
    # async mode
    env = make(fam, 8, batch_size=4)
    with pytest.raises(ValueError, match="selfplay: async mode"):
        env.selfplay(net, record=False)
    with pytest.raises(ValueError, match=r"selfplay_begin: async mode \(batch_size = 4 of num_envs = 8\)"):
        env.device_pool.selfplay_begin(net, record=False)
    env.close()
    # a family without guided search
    env = envpool.make("CartPole-v1", "gymnasium", num_envs=2, seed=1)
    with pytest.raises(RuntimeError, match="guided search not implemented for this environment"):
        env.selfplay(net, record=False)
    with pytest.raises(RuntimeError, match="guided search not implemented for this environment"):
        native.check(env.device_pool._lib.epa_selfplay_begin(env.device_pool._h, h, ctypes.byref(o)))
    env.close()
