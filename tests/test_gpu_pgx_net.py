"""The PGX built-in network on the MI355X: PgxNetEval (envpool_amd/csrc/pgx_net.hip) against the numpy restatement of
the contract (pgx_net_util.py), bit for bit, through the host and the device form of the evaluation -- the CPU cases,
rows that do not fill a wave, F, D and A + 1 that do not fill a tile, and a single layer with an identity-like trunk
and an asymmetric head, which is the check of the int8 matrix-core lane map; `env.evaluate` along the Othello and
ConnectFour fixtures; `run(net)`, the round enqueued from C++, against the same session driven from the host with the
restatement as `evaluate` (Gumbel plain and batch, PUCT plain, wide, and wide with tactics, proofs and two reroots;
a fixed number of advances; a root that is over); a sharded pool; a session with a callable after a net run against a
pool that never saw a net; and the refusals.  k <= 8 roots, S <= 16."""
import ctypes

import numpy as np
import pytest

import envpool_amd as envpool
import pgx_net_util as U
from envpool_amd.core import native
from envpool_amd.core.device_pool import DevicePool
from envpool_amd.pgx.net import Net
from pgx_gumbel_util import gumbel_noise
from pgx_util import ACTIONS, fixture

pytestmark = pytest.mark.gpu

SHAPE = {"TicTacToe": (3, 3, 2), "ConnectFour": (6, 7, 2), "Hex": (11, 11, 4), "Othello": (8, 8, 2)}
FAMILY = {18: "TicTacToe", 84: "ConnectFour", 128: "Othello", 484: "Hex"}  # by F
N, K, OVER = 8, 6, 2  # envs of a pool, roots of a session, the env marked over
IDS = np.array([5, 0, OVER, 7, 3, 1], np.int32)
F32 = np.float32
_pools, _nets = {}, {}


def legal_random(mask, rng):
    mask = np.asarray(mask, bool)
    return (rng.random(mask.shape) * mask + mask).argmax(1).astype(np.int32)


def make_pool(fam, seed=11, pre=3):
    """N envs a few plies into their games, env OVER marked over."""
    pool = DevicePool(fam, N, seed=seed)
    all_ids = np.arange(N, dtype=np.int32)
    rng = np.random.default_rng(2)
    pool.reset(all_ids)
    mask = pool.recv_dict()["info:legal_action_mask"]
    for _ in range(pre):
        pool.send(all_ids, legal_random(mask, rng))
        mask = pool.recv_dict()["info:legal_action_mask"]
    row = pool.get_state([OVER])
    row[0, 1] = 1.0
    pool.set_state(row, [OVER])
    return pool


def get_pool(fam):
    if fam not in _pools:
        _pools[fam] = make_pool(fam)
    pool = _pools[fam]
    if getattr(pool, "_guided_k", None) is not None:
        pool.guided_end()
    return pool


def get_net(fam, d=64, blocks=1, seed=1):
    """(the Net, its layers and scales for the restatement)"""
    key = (fam, d, blocks, seed)
    if key not in _nets:
        f, a = int(np.prod(SHAPE[fam])), ACTIONS[fam]
        layers = U.random_layers(f, a, d, blocks, seed)
        sp, sv = U.scales(d)
        _nets[key] = (Net(SHAPE[fam], a, d, blocks, layers, sp, sv), layers, sp, sv)
    return _nets[key]


def restated(fam, priors, **kw):
    """The restatement as an `evaluate` for the host-driven session."""
    _, layers, sp, sv = get_net(fam, **kw)
    blocks = (len(layers) - 2) // 2

    def evaluate(obs, mask, status):
        return U.restate(layers, blocks, sp, sv, obs, mask, status, priors)

    return evaluate


def same(a, b, where=None):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype, where
        if x.dtype == F32:
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), where
        else:
            assert np.array_equal(x, y), where


def device_eval(pool, net, obs, mask, status, priors):
    import torch

    dev = torch.device("cuda", pool.device)
    t = [torch.as_tensor(x).to(dev) for x in (obs, mask, status)]
    policy, value = net.bind(pool, priors)(*t)
    torch.cuda.synchronize(dev)
    assert policy.dtype == torch.float32 and policy.device == dev
    return policy.cpu().numpy(), value.cpu().numpy()


# -- the kernel against numpy ------------------------------------------------------
@pytest.mark.parametrize("case", U.CASES + [U.LOWERED + (-2,)], ids=str)
def test_kernel_against_numpy(case):
    delta = case[4] if len(case) == 5 else 0
    f, a, d, blocks = case[:4]
    fam = FAMILY[f]
    pool = get_pool(fam)
    layers = U.random_layers(f, a, d, blocks, U.SEEDS[case[:4]], delta)
    sp, sv = U.scales(d)
    net = Net(SHAPE[fam], a, d, blocks, layers, sp, sv)
    for rows in U.ROWS:
        obs, mask, status = U.random_rows(f, a, rows, seed=rows)
        if rows == 100:
            U.check_spread(layers, blocks, obs, lowered=delta != 0)
        for priors in (False, True):
            want = U.restate(layers, blocks, sp, sv, obs, mask, status, priors)
            same(pool.net_eval(net, obs, mask, status, priors), want, (case, rows, priors, "host"))
            same(device_eval(pool, net, obs, mask, status, priors), want, (case, rows, priors, "device"))
    net.close()


def test_single_layer_lane_map():
    """L = 0, W_in = 100 I + a one on the next column, an asymmetric head: h = 100 x[n] + x[n + 1] names every input
    column, and the head's row a weighs column n by (7 a + 13 n) mod 255 - 127, so a swapped or permuted lane map of
    either operand or of the result moves numbers that nothing else in the case can put back."""
    f, a, d = 128, 65, 128
    pool = get_pool("Othello")
    n = np.arange(d)
    w_in = np.zeros((d, f), np.int8)
    w_in[n, n] = 100
    w_in[n, (n + 1) % f] = 1
    w_head = (((7 * np.arange(a + 1)[:, None] + 13 * n[None, :]) % 255) - 127).astype(np.int8)
    assert not np.array_equal(w_head[:a + 1, :a + 1], w_head[:a + 1, :a + 1].T)
    layers = [(w_in, np.arange(d, dtype=np.int32) % 5, 0), (w_head, np.arange(a + 1, dtype=np.int32) * 3 - 50, 0)]
    sp, sv = F32(1.0 / 4096.0), F32(1.0 / 65536.0)
    net = Net(SHAPE["Othello"], a, d, 0, layers, sp, sv)
    rows = 70
    obs = np.zeros((rows, f), np.uint8)
    obs[np.arange(64), 2 * np.arange(64)] = 1      # one input each: a row's answer names its column
    obs[np.arange(64), (37 * np.arange(64) + 5) % f] = 1
    obs[64:] = U.random_rows(f, a, 6, seed=9)[0]
    mask, status = np.ones((rows, a), np.uint8), np.zeros(rows, np.uint8)
    p, _ = U.integers(layers, 0, obs)
    assert len({tuple(r) for r in p.tolist()}) == rows  # every row's integers differ
    for priors in (False, True):
        want = U.restate(layers, 0, sp, sv, obs, mask, status, priors)
        same(pool.net_eval(net, obs, mask, status, priors), want, priors)
    got = pool.net_eval(net, obs, mask, status, False)
    assert np.array_equal(np.rint(got[0].astype(np.float64) * 4096.0).astype(np.int64), p[:, :a])  # the integers
    net.close()


# -- env.evaluate ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Othello-v1", "ConnectFour-v1"])
def test_env_evaluate_along_the_fixture(name):
    g = fixture(name)
    fam = name.split("-")[0]
    n = g["actions"].shape[1]
    net, layers, sp, sv = get_net(fam)
    env = envpool.make(name, "gymnasium", num_envs=n, seed=int(g["seed"]))
    env.reset()
    for t in range(10):
        who = g["info:current_player"][t]
        obs = g["obs"][t][np.arange(n), who]
        status = np.where(g["done"][t] != 0, 2, 0).astype(np.uint8)
        for priors in (False, True):
            want = U.restate(layers, 1, sp, sv, obs, g["info:legal_action_mask"][t], status, priors)
            same(env.evaluate(net, priors=priors), want, (name, t, priors))
        same(env.evaluate(net, [3, 1]), [x[[3, 1]] for x in U.restate(
            layers, 1, sp, sv, obs, g["info:legal_action_mask"][t], status, False)], (name, t))
        env.step(g["actions"][t])
    env.close()


# -- the fused path ----------------------------------------------------------------
def session(env_or_pool, fam, kind, **kw):
    if kind == "gumbel":
        return env_or_pool.gumbel_search(IDS, simulations=12, max_considered=4,
                                         gumbel=gumbel_noise(3, N, ACTIONS[fam])[IDS], **kw)
    return env_or_pool.guided_search(IDS, simulations=12, **kw)


FUSED = [("gumbel", {}), ("gumbel", {"batch": 4}), ("puct", {}), ("puct", {"width": 4})]


@pytest.fixture(scope="module")
def envs():
    """One env per game, a few plies in, env OVER over (through the wrapped pool)."""
    made = {}

    def get(fam):
        if fam not in made:
            env = envpool.make(f"{fam}-v1", "gymnasium", num_envs=N, seed=11)
            rng = np.random.default_rng(2)
            _, info = env.reset()
            for _ in range(3):
                _, _, _, _, info = env.step(legal_random(info["legal_action_mask"], rng))
            pool = env._guided()
            row = pool.get_state([OVER])
            row[0, 1] = 1.0
            pool.set_state(row, [OVER])
            made[fam] = env
        return made[fam]

    yield get
    for env in made.values():
        env.close()


@pytest.mark.parametrize("fam", ["Othello", "ConnectFour"])
@pytest.mark.parametrize("kind,kw", FUSED, ids=str)
def test_run_net_equals_the_host_driven_session(envs, fam, kind, kw):
    env = envs(fam)
    net = get_net(fam)[0]
    host = session(env, fam, kind, **kw)
    first = host.leaves
    want = host.run(restated(fam, priors=kind == "puct"))
    fused = session(env, fam, kind, **kw)
    same(fused.leaves, first)
    got = fused.run(net)
    same(got, want, (fam, kind, kw))
    assert fused.calls == host.calls and fused._pool is None and got._fields == want._fields
    assert got.action[list(IDS).index(OVER)] == -1 and not got.visits[list(IDS).index(OVER)].any()  # the root that is over
    assert got.visits.sum() == (K - 1) * 12


def test_run_net_with_tactics_proofs_and_two_reroots(envs):
    fam = "ConnectFour"
    env, net = envs(fam), get_net(fam)[0]
    kw = dict(width=4, tactics=1, prove=True, nodes=40)
    out = []
    for evaluate in (restated(fam, True), net):
        gs = session(env, fam, "puct", **kw)
        rounds = [gs.run(evaluate, close=False)]
        for _ in range(2):
            action = np.where(rounds[-1].action < 0, 0, rounds[-1].action).astype(np.int32)
            gs.reroot(action, 8)
            rounds.append(gs.run(evaluate, close=False))
        out.append((rounds, gs.proof, gs.decided, gs.leaves, gs.calls))
        gs.close()
    for a, b in zip(out[0][0], out[1][0]):
        same(a, b)
    same(out[0][1], out[1][1])
    assert np.array_equal(out[0][2], out[1][2]) and out[0][4] == out[1][4]
    same(out[0][3], out[1][3])


@pytest.mark.parametrize("kind", ["gumbel", "puct"])
def test_a_fixed_number_of_advances(kind):
    fam = "Othello"
    pool, (net, layers, sp, sv) = get_pool(fam), get_net(fam)
    noise = gumbel_noise(3, N, ACTIONS[fam])[IDS]

    def begin():
        if kind == "gumbel":
            return pool.gumbel_begin(noise, IDS, 12, 4, batch=4)
        return pool.guided_begin(IDS, 12, width=4)

    advance, result = (pool.gumbel_advance, pool.gumbel_result) if kind == "gumbel" else \
        (pool.guided_advance, pool.guided_result)
    leaves = begin()
    for _ in range(3):
        flat = (leaves[0].reshape((-1,) + SHAPE[fam]), leaves[1].reshape(-1, ACTIONS[fam]), leaves[2].reshape(-1))
        leaves = advance(*U.restate(layers, 1, sp, sv, *flat, kind == "puct"))
    want = (leaves, result())
    got_leaves, made = pool.net_run(net, begin(), advances=3)
    assert made == 3
    same(got_leaves, want[0])
    same(result(), want[1])
    # the rest of the round, then nothing is left to do
    rest, more = pool.net_run(net, got_leaves)
    assert (rest[2] == 2).all() and 1 <= more <= 10
    assert pool.net_run(net, rest)[1] == 0
    with pytest.raises(ValueError, match="net_run: advances = 13 must be 0 .. "):
        pool.net_run(net, rest, advances=13)
    pool.guided_end()


def test_device_forms_take_the_net():
    import torch

    from envpool_amd.torch_interop import gumbel_search_device, guided_reroot_device, guided_search_device

    fam = "Othello"
    pool, net = get_pool(fam), get_net(fam)[0]
    dev = torch.device("cuda", pool.device)
    noise = gumbel_noise(3, N, ACTIONS[fam])[IDS]
    pool.net_run(net, pool.gumbel_begin(noise, IDS, 12, 4, batch=4))
    want = pool.gumbel_result()
    pool.guided_end()
    got = gumbel_search_device(pool, net, IDS, 12, 4, gumbel=torch.as_tensor(noise).to(dev), batch=4)
    same([t.cpu().numpy() for t in got], want)
    # PUCT with a reroot: the callable form of the same net on the device against the shortcut
    out = []
    for evaluate in (net.bind(pool, priors=True), net):
        first = guided_search_device(pool, evaluate, IDS, 12, nodes=40, keep_open=True)
        action = torch.where(first[2] < 0, torch.zeros_like(first[2]), first[2])
        second = guided_reroot_device(pool, evaluate, action, 8)
        out.append([t.cpu().numpy() for t in first + second])
        pool.guided_end()
    same(out[0], out[1])


def test_sharded_pool_equals_the_unsharded():
    fam = "ConnectFour"
    net = get_net(fam)[0]
    results = []
    for device in ([0, 0], 0):
        env = envpool.make(f"{fam}-v1", "gymnasium", num_envs=N, device=device, seed=11)
        rng = np.random.default_rng(2)
        _, info = env.reset()
        for _ in range(3):
            _, _, _, _, info = env.step(legal_random(info["legal_action_mask"], rng))
        rows = []
        for kind, kw in FUSED:
            gs = session(env, fam, kind, **kw)
            rows.append(gs.run(net))
        rows.append(env.evaluate(net, IDS, priors=True))
        results.append(rows)
        env.close()
    for a, b in zip(*results):
        same(a, b)


def test_a_callable_after_a_net_run_gives_what_it_gave():
    fam = "Othello"
    net = get_net(fam)[0]
    evaluate = restated(fam, True, seed=2)  # another network's numbers
    out = []
    for with_net in (True, False):
        pool = make_pool(fam, seed=5)
        env_like = pool
        if with_net:
            leaves = pool.guided_begin(IDS, 12, width=4)
            pool.net_run(net, leaves)
            pool.guided_end()
            pool.net_eval(net, *[x.reshape((-1,) + x.shape[2:]) for x in leaves])
        leaves = env_like.guided_begin(IDS, 12)
        rec = [leaves]
        for _ in range(13):
            leaves = pool.guided_advance(*evaluate(*leaves))
            rec.append(leaves)
        rec.append(pool.guided_result())
        pool.guided_end()
        out.append((rec, pool.get_state()))
        pool.close()
    for a, b in zip(out[0][0], out[1][0]):
        same(a, b)
    assert np.array_equal(out[0][1], out[1][1])


# -- refusals ----------------------------------------------------------------------
def test_refusals():
    pool = get_pool("Othello")
    net = get_net("Othello")[0]
    other = get_net("ConnectFour")[0]
    obs, mask, status = U.random_rows(128, 65, 4, seed=1)
    with pytest.raises(ValueError, match="net_eval: a net of F = 84, A = 7 for a pool of F = 128, A = 65"):
        native.check(pool._lib.epa_net_eval(pool._h, other._handle(pool.device), 4, 0, obs.ctypes.data,
                                            mask.ctypes.data, status.ctypes.data, obs.ctypes.data, obs.ctypes.data))
    leaves = pool.guided_begin(IDS, 8)
    with pytest.raises(ValueError, match="net_run: a net of F = 84, A = 7 for a pool of F = 128, A = 65"):
        pool.net_run(other, leaves)
    # same F, another A
    odd = Net(SHAPE["Othello"], 64, 32, 0, U.random_layers(128, 64, 32, 0, 1), *U.scales(32))
    with pytest.raises(ValueError, match="a net of F = 128, A = 64 for a pool of F = 128, A = 65"):
        pool.net_run(odd, leaves)
    pool.guided_end()
    with pytest.raises(ValueError, match="net_run: the pool has no guided-search session"):
        pool.net_run(net, leaves)
    made = ctypes.c_int32(0)
    with pytest.raises(ValueError, match="net_run: the pool has no guided-search session"):
        native.check(pool._lib.epa_net_run(pool._h, net._handle(pool.device), 0, leaves[0].ctypes.data,
                                           leaves[1].ctypes.data, leaves[2].ctypes.data, ctypes.byref(made)))
    # a device index that is no device of this machine; a net of another device, where there is one
    blob, out = net.blob(), ctypes.c_void_p()
    count = native.device_count()
    for device in (-1, count):
        with pytest.raises(ValueError, match=f"net_create: device = {device} must be 0 .. {count - 1}"):
            native.check(pool._lib.epa_net_create(device, blob.ctypes.data, blob.nbytes, ctypes.byref(out)))
    if count > 1:
        with pytest.raises(ValueError, match="net_eval: the net is on device 1, the pool on device 0"):
            native.check(pool._lib.epa_net_eval(pool._h, net._handle(1), 4, 0, obs.ctypes.data, mask.ctypes.data,
                                                status.ctypes.data, obs.ctypes.data, obs.ctypes.data))
    bad = blob.copy()
    bad[12] = 1  # A = 1 + 65 - 65 ...: the sizes no longer give the blob's length
    with pytest.raises(ValueError, match="net: a blob of"):
        native.check(pool._lib.epa_net_create(0, bad.ctypes.data, bad.nbytes, ctypes.byref(out)))
    for rows, mode in ((0, 0), (4, 2)):
        with pytest.raises(ValueError, match="net_eval: (rows|mode)"):
            native.check(pool._lib.epa_net_eval(pool._h, net._handle(pool.device), rows, mode, obs.ctypes.data,
                                                mask.ctypes.data, status.ctypes.data, obs.ctypes.data,
                                                obs.ctypes.data))
    with pytest.raises(ValueError, match="net_eval: obs"):
        pool.net_eval(net, obs[:, :100], mask, status)


OTHERS = ["CartPole-v1", "Pendulum-v1", "MountainCar-v0", "MountainCarContinuous-v0", "Acrobot-v1", "Catch-v0",
          "FrozenLake-v1", "Taxi-v3", "NChain-v0", "CliffWalking-v0", "Blackjack-v1", "HalfCheetah-v4", "Ant-v4",
          "Walker2d-v4", "InvertedPendulum-v4", "InvertedDoublePendulum-v4", "Reacher-v4", "Swimmer-v4", "Hopper-v4",
          "Humanoid-v4", "HumanoidStandup-v4", "Pusher-v4", "MiniGrid-Empty-5x5-v0", "Game2048-v1", "Minesweeper-v0",
          "SlidingTilePuzzle-v0", "RubiksCube-v0", "Snake-v1", "Maze-v0"]


def test_every_other_family_refuses():
    """One task of every native family that is no PGX game: the Python entry points and the raw calls."""
    net = get_net("TicTacToe", d=32, blocks=0)[0]
    names = {native.lib().epa_family_name(i).decode() for i in range(native.lib().epa_num_families())}
    seen = set()
    buf = np.zeros(256, np.uint8)
    for task in OTHERS:
        env = envpool.make(task, "gymnasium", num_envs=2, seed=1)
        pool = env._guided()
        seen.add(pool.family)
        with pytest.raises(RuntimeError, match="guided search not implemented for this environment"):
            env.evaluate(net)
        with pytest.raises(RuntimeError, match="guided search not implemented for this environment"):
            pool.net_run(net, (buf, buf, buf))
        for call in (lambda: pool._lib.epa_net_eval(pool._h, net._handle(pool.device), 1, 0, buf.ctypes.data,
                                                    buf.ctypes.data, buf.ctypes.data, buf.ctypes.data,
                                                    buf.ctypes.data),
                     lambda: pool._lib.epa_net_run_device(pool._h, net._handle(pool.device), 0, buf.ctypes.data,
                                                          buf.ctypes.data, buf.ctypes.data, None)):
            with pytest.raises(RuntimeError, match="guided search not implemented for this environment"):
                native.check(call())
        env.close()
    assert seen == names - set(SHAPE)
