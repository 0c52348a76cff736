"""The PGX convolutional network on the MI355X: PgxConvEval (envpool_amd/csrc/pgx_conv.hip) against the numpy
restatement (pgx_conv_util.py), bit for bit, through both forms of the evaluation; `run(net)` against the same session
driven from the host with the restatement as `evaluate`; `evaluate_pair` of two ConvNets; and the refusals."""
import functools

import numpy as np
import pytest

import envpool_amd as envpool
import pgx_conv_util as U
from envpool_amd.core.device_pool import DevicePool
from envpool_amd.pgx.net import ConvNet, Net
from pgx_gumbel_util import gumbel_noise
from pgx_net_util import random_rows
from pgx_util import ACTIONS

pytestmark = pytest.mark.gpu

FAMILY = {(3, 3, 2): "TicTacToe", (6, 7, 2): "ConnectFour", (11, 11, 4): "Hex", (8, 8, 2): "Othello"}
N, OVER = 8, 2  # envs of a pool, the env marked over
IDS = np.array([5, 0, OVER, 7, 3, 1], np.int32)


@functools.lru_cache(None)
def get_pool(fam):
    return DevicePool(fam, N, seed=11)


def make_net(case, seed=0, shift_delta=0):
    """(the ConvNet, the restatement as an `evaluate(obs, mask, status, priors)`)"""
    h, w, c, a, d, blocks, p = case
    layers = U.random_layers(*case, seed, shift_delta)
    sp, sv = U.scales(h, w, p)

    def evaluate(obs, mask, status, priors):
        return U.restate(layers, blocks, (h, w, c), sp, sv, obs, mask, status, priors)

    return ConvNet((h, w, c), a, d, blocks, p, layers, sp, sv), evaluate


def same(a, b, where=None):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype, where
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                              y.view(np.uint32) if y.dtype == np.float32 else y), where


def device_eval(pool, net, obs, mask, status, priors):
    import torch

    dev = torch.device("cuda", pool.device)
    policy, value = net.bind(pool, priors)(*[torch.as_tensor(x).to(dev) for x in (obs, mask, status)])
    torch.cuda.synchronize(dev)
    return policy.cpu().numpy(), value.cpu().numpy()


@pytest.mark.parametrize("case", U.ALL, ids=str)
def test_kernel_against_numpy(case):
    delta, case = case[7], case[:7]
    h, w, c, a = case[:4]
    pool = get_pool(FAMILY[(h, w, c)])
    net, evaluate = make_net(case, U.SEEDS[case], delta)
    for rows in U.ROWS:
        obs, mask, status = random_rows(h * w * c, a, rows, seed=rows)
        for priors in (False, True):
            want = evaluate(obs, mask, status, priors)
            same(pool.net_eval(net, obs, mask, status, priors), want, (case, rows, priors, "host"))
            same(device_eval(pool, net, obs, mask, status, priors), want, (case, rows, priors, "device"))
    net.close()


@pytest.mark.parametrize("fam,case", [("Othello", (8, 8, 2, 65, 64, 1, 4)), ("TicTacToe", (3, 3, 2, 9, 32, 1, 4))])
@pytest.mark.parametrize("kind,kw", [("gumbel", {"batch": 4}), ("puct", {"width": 4})], ids=str)
def test_run_net_equals_the_host_driven_session(fam, case, kind, kw):
    """k = 6 roots a few plies in, one of them over, 16 simulations."""
    env = envpool.make(f"{fam}-v1", "gymnasium", num_envs=N, seed=11)
    rng = np.random.default_rng(2)
    _, info = env.reset()
    for _ in range(2):
        legal = np.asarray(info["legal_action_mask"], bool)
        _, _, _, _, info = env.step((rng.random(legal.shape) * legal + legal).argmax(1).astype(np.int32))
    pool = env._guided()
    row = pool.get_state([OVER])
    row[0, 1] = 1.0
    pool.set_state(row, [OVER])
    net, evaluate = make_net(case, seed=1)

    def session():
        if kind == "gumbel":
            return env.gumbel_search(IDS, simulations=16, max_considered=4,
                                     gumbel=gumbel_noise(3, N, ACTIONS[fam])[IDS], **kw)
        return env.guided_search(IDS, simulations=16, **kw)

    host = session()
    want = host.run(lambda obs, mask, status: evaluate(obs, mask, status, kind == "puct"))
    fused = session()
    got = fused.run(net)
    same(got, want, (fam, kind))
    assert fused.calls == host.calls and got.action[list(IDS).index(OVER)] == -1
    env.close()
    net.close()


def test_evaluate_pair_equals_evaluate_of_the_named_net():
    env = envpool.make("Othello-v1", "gymnasium", num_envs=100, seed=3)
    env.reset()
    a, _ = make_net((8, 8, 2, 65, 64, 2, 8), seed=1)
    b, _ = make_net((8, 8, 2, 65, 32, 0, 4), seed=2)
    for priors in (False, True):
        ea, eb = env.evaluate(a, priors=priors), env.evaluate(b, priors=priors)
        for side in (np.zeros(100, np.uint8), np.ones(100, np.uint8), (np.arange(100) * 7 % 3 == 0).astype(np.uint8)):
            pick = side.astype(bool)
            same(env.evaluate_pair(a, b, side, priors=priors),
                 (np.where(pick[:, None], eb[0], ea[0]), np.where(pick, eb[1], ea[1])), (priors, side[:8]))
    env.close()


def test_refusals():
    pool = get_pool("Othello")
    conv, _ = make_net((8, 8, 2, 65, 32, 0, 4))
    dense = Net.random((8, 8, 2), 65, 32, 0, seed=1)
    obs, mask, status = random_rows(128, 65, 4, seed=1)
    side = np.array([0, 1, 1, 0], np.uint8)
    with pytest.raises(ValueError, match="net_eval_pair: net_a is a ConvNet and net_b a Net: the two nets of a pair"):
        pool.net_eval_pair(conv, dense, obs, mask, status, side)
    # the pool's F and A, another board: H, W and C each
    for shape in ((4, 16, 2), (16, 4, 2), (8, 4, 4)):
        other, _ = make_net(shape + (65, 32, 0, 4))
        with pytest.raises(ValueError, match=rf"net_eval: a conv net of \[{shape[0]}, {shape[1]}, {shape[2]}\] for a "
                                             r"pool of \[8, 8, 2\]"):
            pool.net_eval(other, obs, mask, status)
