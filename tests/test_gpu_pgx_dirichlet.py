"""PUCT exploration of the PGX self-play driver on the MI355X: the noise rows of PgxSelfplayDirichlet against the numpy
restatement (pgx_dirichlet_util), bit for bit; `env.selfplay(net, policy="puct", dirichlet_alpha=, temperature=)` and
the arena against the same plies driven from Python -- the roots evaluated with the bound net, the restatement's eta
mixed in numpy, the round finished with `run(net)`, the restated move --, sample for sample, byte for byte; the plain
driver through `epa_selfplay_begin_ex`; continuation, seeds, a sharded pool, the torch form; every refusal."""
import ctypes

import numpy as np
import pytest

import pgx_arena_util as AU
import pgx_dirichlet_util as D
import pgx_selfplay_util as U
from envpool_amd.core import native
from envpool_amd.python.envpool import ArenaStats
from test_gpu_pgx_arena import nets_of
from test_gpu_pgx_selfplay import ACTIONS, Run, make, net_of, same_per_env, same_runs, search_kw, state_of

pytestmark = pytest.mark.gpu

F = np.float32


def bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def split(kw):
    env_kw = {k: v for k, v in kw.items() if k in ("env_id_offset", "device")}
    return env_kw, {k: v for k, v in kw.items() if k not in env_kw}


def root_masks(env):
    """The legal actions [N, A] and statuses [N] of the envs' current positions (a one-simulation session's leaves)."""
    gs = env.guided_search(simulations=1)
    _, mask, status = gs.leaves
    gs.close()
    return np.asarray(mask), np.asarray(status)


# -- the noise rows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,n,plies,kw", [
    ("TicTacToe", 65, 10, dict(env_id_offset=3)),      # rows that do not fill the last wave; roots that are over
    ("Othello", 64, 2, dict()),                        # two actions per lane
    ("Hex", 33, 2, dict(width=2)),                     # two actions per lane, the roots' rows are slot 0 of two
    ("ConnectFour", 1, 2, dict()),                     # one row, a group of 8 lanes
], ids=lambda x: str(x).replace(" ", ""))
def test_noise_rows_equal_the_restatement(fam, n, plies, kw):
    env_kw, opts = split(kw)
    env = make(fam, n, **env_kw)
    env.reset()
    ids = np.asarray(env.all_env_ids)
    assert ids[0] == env_kw.get("env_id_offset", 0)
    sp = env.selfplay(net_of(fam), policy="puct", simulations=4, seed=9, record=False, dirichlet_alpha=0.3, **opts)
    assert sp.noise().shape == (n, ACTIONS[fam]) and not sp.noise().any()  # zeros before the first ply
    over = 0
    for t in range(plies):
        mask, status = root_masks(env)  # (replaces the driver's session, which opens its own each ply)
        sp.run(1)
        want, fallbacks = D.eta_rows(9, ids, t, mask, 0.3)
        got = sp.noise()
        assert got.dtype == F and np.array_equal(bits(got), bits(want)), (fam, t)
        assert fallbacks == 0 and (got[mask] > 0).all() and not got[~mask].any()
        over += int((status != 0).sum())
        assert not got[status != 0].any()  # a root that is over has no legal action and a zero row
    if fam == "TicTacToe":
        assert over > 0  # some game ended within these plies: the zero rows were exercised
    sp.close()
    env.close()


def test_gumbel_noise_rows_read_out():
    env = make("TicTacToe", 10, env_id_offset=2)
    env.reset()
    sp = env.selfplay(net_of("TicTacToe"), simulations=4, seed=9, record=False, max_considered=4)
    sp.run(2)
    assert np.array_equal(bits(sp.noise()), bits(U.noise_rows(9, env.all_env_ids, 1, 9)))
    sp.close()
    env.close()


# -- the driver against the host-driven loop ---------------------------------------------------------------------------
def driver_run(fam, n, plies, seed=5, simulations=8, parts=None, **kw):
    env_kw, opts = split(kw)
    env = make(fam, n, **env_kw)
    rec = env.recorder(capacity=1 << 15)
    env.reset()
    sp = env.selfplay(net_of(fam), policy="puct", simulations=simulations, seed=seed, **opts)
    for p in parts or [plies]:
        stats = sp.run(p)
    out = Run(rec.drain(), rec.counters, state_of(env), stats)
    sp.close()
    rec.close()
    env.close()
    return out


def noisy_round(env, evaluate, finish, ids, t, seed, simulations, opts):
    """One search round with the restatement's eta mixed into the roots' priors: the first evaluation and advance by
    hand, the rest of the round by `finish` (the net itself: enqueued from C++; a callable: from Python)."""
    gs = env.guided_search(simulations=simulations, **search_kw("puct", opts))
    obs, mask, status = gs.leaves
    a = mask.shape[-1]
    priors, values = evaluate(obs.reshape((-1,) + obs.shape[-3:]), mask.reshape(-1, a), status.reshape(-1))
    priors, values = np.array(priors, F).reshape(mask.shape), np.asarray(values, F).reshape(status.shape)
    alpha, eps = opts.get("dirichlet_alpha", 0.0), opts.get("dirichlet_eps", 0.25)
    if alpha > 0:
        wide = mask.ndim == 3  # the root's own row is slot 0
        m0, s0 = (mask[:, 0], status[:, 0]) if wide else (mask, status)
        eta, _ = D.eta_rows(seed, ids, t, m0, alpha)
        mixed = D.mix(priors[:, 0] if wide else priors, eta, m0, s0, eps)
        if wide:
            priors[:, 0] = mixed
        else:
            priors = mixed
    gs.advance(priors, values)
    return gs.run(finish)


def host_run(fam, n, plies, seed=5, simulations=8, **kw):
    env_kw, opts = split(kw)
    env = make(fam, n, **env_kw)
    net = net_of(fam)
    evaluate = net.bind(env, priors=True)
    rec = env.recorder(capacity=1 << 15)
    _, info = env.reset()
    ids = np.asarray(env.all_env_ids)
    elapsed = np.asarray(info["elapsed_step"]).reshape(-1)
    total = np.zeros(5, np.int64)
    for t in range(plies):
        result = noisy_round(env, evaluate, net, ids, t, seed, simulations, opts)
        action, target = D.puct_move_temp(result.visits, result.action, elapsed, opts.get("sample_plies", 0),
                                          U.key(seed, ids, t), opts.get("temperature", 1.0))
        rec.add(target)
        _, rew, term, trunc, info = env.step(action)
        rec.finish(rew, term | trunc)
        elapsed = np.asarray(info["elapsed_step"]).reshape(-1)
        total += U.tally(term | trunc, rew, elapsed)
    out = Run(rec.drain(), rec.counters, state_of(env), tuple(int(x) for x in total) + (plies,))
    rec.close()
    env.close()
    return out


CONFIGS = [
    ("TicTacToe", 48, 12, 16, dict(dirichlet_alpha=0.3, sample_plies=4, temperature=0.5)),
    ("ConnectFour", 48, 8, 8, dict(dirichlet_alpha=0.3, sample_plies=4, temperature=2.0, width=2)),
    ("Othello", 24, 4, 8, dict(dirichlet_alpha=0.3, dirichlet_eps=0.5, sample_plies=2, temperature=0.25)),
    ("Hex", 24, 3, 8, dict(dirichlet_alpha=1.0, sample_plies=3, temperature=0.5, width=2)),
]


@pytest.mark.parametrize("fam,n,plies,simulations,opts", CONFIGS, ids=lambda x: str(x).replace(" ", ""))
def test_driver_equals_the_host_driven_loop(fam, n, plies, simulations, opts):
    got = driver_run(fam, n, plies, simulations=simulations, **opts)
    want = host_run(fam, n, plies, simulations=simulations, **opts)
    same_runs(got, want, (fam, opts))
    assert got.stats.t == plies
    assert np.allclose(got.samples.policy.sum(axis=1), 1.0, atol=1e-5)  # the target stays visits / V
    if fam == "TicTacToe":
        assert got.stats.games >= n  # every env finished a game: resets and roots that are over were played through
    # the noise matters: the plain driver plays other games
    plain = driver_run(fam, n, plies, simulations=simulations, sample_plies=opts["sample_plies"],
                       **search_kw("puct", opts))
    assert not np.array_equal(plain.state, got.state)


def test_eps_zero_draws_and_changes_nothing():
    plain = driver_run("TicTacToe", 32, 10, sample_plies=3)
    quiet = driver_run("TicTacToe", 32, 10, sample_plies=3, dirichlet_alpha=0.3, dirichlet_eps=0.0)
    same_runs(plain, quiet)


def test_begin_ex_with_the_plain_extra_is_the_plain_driver():
    fam, n = "ConnectFour", 40
    runs = []
    for ex in (False, True):
        env = make(fam, n)
        pool = env.device_pool
        rec = env.recorder(capacity=1 << 15)
        env.reset()
        o = native.check_selfplay(policy="puct", simulations=8, seed=5, sample_plies=4, width=2)
        h = net_of(fam)._handle(pool.device)
        if ex:
            x = native.SelfplayExtra(0.0, 0.0, 1.0, 0)
            native.check(pool._lib.epa_selfplay_begin_ex(pool._h, h, None, ctypes.byref(o), ctypes.byref(x)))
        else:
            native.check(pool._lib.epa_selfplay_begin(pool._h, h, ctypes.byref(o)))
        pool.selfplay_run(8)
        runs.append(Run(rec.drain(), rec.counters, state_of(env), tuple(int(v) for v in pool.selfplay_stats())))
        assert not pool.selfplay_noise().any()
        pool.selfplay_end()
        rec.close()
        env.close()
    same_runs(runs[0], runs[1])


def test_continuation_and_seeds():
    opts = dict(dirichlet_alpha=0.3, sample_plies=2, temperature=0.5)
    whole = driver_run("TicTacToe", 32, 5, **opts)
    parts = driver_run("TicTacToe", 32, 5, parts=[3, 2], **opts)
    same_runs(whole, parts)
    assert parts.stats.t == 5
    # nothing but the noise depends on the seed here (no sampled ply)
    loud = [driver_run("TicTacToe", 32, 6, seed=s, dirichlet_alpha=0.3) for s in (1, 2)]
    assert not np.array_equal(loud[0].state, loud[1].state)
    assert loud[0].samples.policy.tobytes() != loud[1].samples.policy.tobytes()


def test_sharded_pool_plays_the_unsharded_pools_games():
    opts = dict(dirichlet_alpha=0.3, sample_plies=4, temperature=0.5, width=2)
    one = driver_run("TicTacToe", 32, 12, **opts)
    two = driver_run("TicTacToe", 32, 12, device=[0, 0], **opts)
    same_per_env(one, two, 32)
    # ... and reads out the unsharded pool's noise rows
    noise = []
    for kw in (dict(), dict(device=[0, 0])):
        env = make("TicTacToe", 32, **kw)
        env.reset()
        sp = env.selfplay(net_of("TicTacToe"), policy="puct", simulations=4, seed=5, record=False, dirichlet_alpha=0.3)
        sp.run(1)
        noise.append(sp.noise())
        sp.close()
        env.close()
    assert noise[0].any() and np.array_equal(bits(noise[0]), bits(noise[1]))


def test_torch_form_equals_the_host_form():
    import torch

    from envpool_amd.torch_interop import selfplay_device

    fam = "Othello"
    opts = dict(dirichlet_alpha=0.3, sample_plies=2, temperature=0.5, width=2)
    want = driver_run(fam, 24, 5, **opts)
    env = make(fam, 24)
    pool = env.device_pool
    rec = env.recorder(capacity=1 << 15)
    env.reset()
    dev = torch.device("cuda", pool.device)
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        selfplay_device(pool, net_of(fam), 3, policy="puct", simulations=8, seed=5, **opts)
        selfplay_device(pool, net_of(fam), 2)  # the open driver continues
        torch.cuda.current_stream(dev).synchronize()
    stats = pool.selfplay_stats()
    same_runs(Run(rec.drain(), rec.counters, state_of(env), tuple(int(x) for x in stats)), want)
    pool.selfplay_end()
    env.close()


# -- the arena -------------------------------------------------------------------------------------------------------
def test_arena_equals_the_two_net_host_loop():
    fam, n, plies, seed = "TicTacToe", 48, 12, 5
    opts = dict(dirichlet_alpha=0.3, sample_plies=4, temperature=0.5, width=2)
    a = ACTIONS[fam]
    net_a, net_b = nets_of(fam)
    env = make(fam, n)
    rec = env.recorder(capacity=1 << 15)
    env.reset()
    arena = env.arena(net_a, net_b, policy="puct", simulations=8, seed=seed, record=True, **opts)
    stats = arena.run(plies)
    got = Run(rec.drain(), rec.counters, state_of(env), stats)
    arena.close()
    env.close()

    env = make(fam, n)
    both = [net.bind(env, True) for net in (net_a, net_b)]
    rec = env.recorder(capacity=1 << 15)
    _, info = env.reset()
    ids = np.asarray(env.all_env_ids)
    elapsed = np.asarray(info["elapsed_step"]).reshape(-1)
    total = np.zeros(7, np.int64)
    for t in range(plies):
        side = AU.net_of(ids, np.asarray(info["current_player"]).reshape(-1))  # fixed for the ply

        def evaluate(obs, mask, status):
            (pa, va), (pb, vb) = (ev(obs, mask, status) for ev in both)
            s = np.repeat(side, pa.reshape(-1, a).shape[0] // n).astype(bool)
            return (np.where(s[:, None], pb.reshape(-1, a), pa.reshape(-1, a)).reshape(pa.shape),
                    np.where(s, vb.reshape(-1), va.reshape(-1)).reshape(va.shape))

        result = noisy_round(env, evaluate, evaluate, ids, t, seed, 8, opts)
        action, target = D.puct_move_temp(result.visits, result.action, elapsed, 4, U.key(seed, ids, t), 0.5)
        rec.add(target)
        _, rew, term, trunc, info = env.step(action)
        rec.finish(rew, term | trunc)
        elapsed = np.asarray(info["elapsed_step"]).reshape(-1)
        total += AU.tally(term | trunc, rew, elapsed, ids)
    want = Run(rec.drain(), rec.counters, state_of(env), ArenaStats(*(int(x) for x in total), plies))
    env.close()
    same_runs(got, want)
    assert got.stats.games >= n and got.stats.wins_a + got.stats.wins_b + got.stats.draws == got.stats.games


# -- refusals --------------------------------------------------------------------------------------------------------
def test_refusals():
    fam = "TicTacToe"
    net = net_of(fam)
    net_a, net_b = nets_of(fam)
    env = make(fam, 8)
    env.reset()
    pool = env.device_pool
    with pytest.raises(ValueError, match="selfplay_noise: the pool has no self-play driver"):
        pool.selfplay_noise()
    for kw, msg in [
        (dict(dirichlet_alpha=-1.0), "selfplay: dirichlet_alpha = -1.0 must be finite and in 0 .. 100"),
        (dict(dirichlet_alpha=101), "selfplay: dirichlet_alpha = 101 must be finite and in 0 .. 100"),
        (dict(dirichlet_alpha=float("nan")), "selfplay: dirichlet_alpha = nan must be finite"),
        (dict(dirichlet_alpha=0.3, dirichlet_eps=1.5), "selfplay: dirichlet_eps = 1.5 must be in 0 .. 1"),
        (dict(dirichlet_eps=-0.5), "selfplay: dirichlet_eps = -0.5 must be in 0 .. 1"),
        (dict(temperature=0.01), "selfplay: temperature = 0.01 must be in 0.05 .. 20"),
        (dict(temperature=21), "selfplay: temperature = 21 must be in 0.05 .. 20"),
    ]:
        with pytest.raises(ValueError, match=msg):
            env.selfplay(net, policy="puct", record=False, **kw)
        with pytest.raises(ValueError, match=msg):
            env.arena(net_a, net_b, policy="puct", **kw)
        with pytest.raises(ValueError, match=msg):
            pool.selfplay_begin(net, policy="puct", record=False, **kw)
    for kw in (dict(dirichlet_alpha=0.3), dict(dirichlet_eps=0.5), dict(temperature=0.5)):
        with pytest.raises(ValueError, match=rf"selfplay: \['{list(kw)[0]}'\] are arguments of policy='puct'"):
            env.selfplay(net, record=False, max_considered=4, **kw)
        with pytest.raises(ValueError, match="are arguments of policy='puct'"):
            env.arena(net_a, net_b, max_considered=4, **kw)
    # the engine's own refusals, through the raw call: what the Python checks would have stopped
    h, ha, hb = (x._handle(pool.device) for x in (net, net_a, net_b))

    def raw(policy, alpha=0.0, eps=0.0, temperature=1.0, reserved=0, arena=False):
        o = native.check_selfplay(policy=policy, record=False, simulations=4)
        x = native.SelfplayExtra(alpha, eps, temperature, reserved)
        nets = (ha, hb) if arena else (h, None)
        return pool._lib.epa_selfplay_begin_ex(pool._h, *nets, ctypes.byref(o), ctypes.byref(x))

    for arena in (False, True):
        what = "arena_begin" if arena else "selfplay_begin"
        for kw, msg in [
            (dict(alpha=-0.5), f"{what}: dirichlet_alpha = -0.5.* must be finite and in 0 .. 100"),
            (dict(alpha=100.5), f"{what}: dirichlet_alpha = 100.5.* must be finite and in 0 .. 100"),
            (dict(alpha=float("nan")), f"{what}: dirichlet_alpha = .*nan must be finite and in 0 .. 100"),
            (dict(alpha=float("inf")), f"{what}: dirichlet_alpha = inf must be finite and in 0 .. 100"),
            (dict(alpha=0.3, eps=-0.25), f"{what}: dirichlet_eps = -0.25.* must be in 0 .. 1"),
            (dict(alpha=0.3, eps=1.25), f"{what}: dirichlet_eps = 1.25.* must be in 0 .. 1"),
            (dict(eps=float("nan")), f"{what}: dirichlet_eps = .*nan must be in 0 .. 1"),
            (dict(temperature=0.04), f"{what}: temperature = 0.04.* must be in 0.05 .. 20"),
            (dict(temperature=20.5), f"{what}: temperature = 20.5.* must be in 0.05 .. 20"),
            (dict(temperature=float("nan")), f"{what}: temperature = .*nan must be in 0.05 .. 20"),
            (dict(reserved=1), f"{what}: the extra options' reserved must be 0"),
        ]:
            with pytest.raises(ValueError, match=msg):
                native.check(raw("puct", arena=arena, **kw))
        for kw, name in [(dict(alpha=0.3), "dirichlet_alpha"), (dict(eps=0.25), "dirichlet_eps"),
                         (dict(temperature=0.5), "temperature"), (dict(temperature=float("nan")), "temperature")]:
            with pytest.raises(ValueError, match=f"{what}: {name} is an argument of the PUCT policy"):
                native.check(raw("gumbel", arena=arena, **kw))
    o = native.check_selfplay(policy="puct", record=False, simulations=4)
    x = native.SelfplayExtra(0.3, 0.25, 1.0, 0)
    with pytest.raises(ValueError, match="selfplay_begin: null argument"):
        native.check(pool._lib.epa_selfplay_begin_ex(pool._h, h, None, ctypes.byref(o), None))
    with pytest.raises(ValueError, match="selfplay_begin: null argument"):
        native.check(pool._lib.epa_selfplay_begin_ex(pool._h, None, None, ctypes.byref(o), ctypes.byref(x)))
    with pytest.raises(ValueError, match="selfplay_noise: the pool has no self-play driver"):  # nothing was opened
        pool.selfplay_noise()
    # what is allowed: alpha > 0 with eps == 0, the ends of the ranges
    for kw in (dict(alpha=0.3), dict(alpha=100.0, eps=1.0, temperature=20.0), dict(temperature=0.05)):
        native.check(raw("puct", **kw))
        pool.selfplay_run(1)
    native.check(raw("gumbel"))
    with pytest.raises(ValueError, match="selfplay_noise: null argument"):
        native.check(pool._lib.epa_selfplay_noise(pool._h, None))
    pool.selfplay_end()
    env.close()
