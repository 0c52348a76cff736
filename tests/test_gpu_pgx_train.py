"""Training kernels of the PGX built-in network on the device (csrc/pgx_train.hip) against the float64 twin
`Net.module()` with autograd on the CPU: the forward integers exactly, every gradient within m c G_abs (the contract
header derives c; G_abs is the same backward pass over |W|, |dp| and the same masks; m the layers up to the output),
at the shapes where the tiling can go wrong; the crafted boundary net; bit-identical repeats; an Actor's `logp` and
`value`; and the C-level refusals."""
import ctypes

import numpy as np
import pytest
import torch

import pgx_train_util as U
from envpool_amd.actor import Actor
from envpool_amd.core import native
from envpool_amd.pgx import train
from envpool_amd.pgx.net import Net

pytestmark = pytest.mark.gpu
# (rows, F, D, L, A, binary inputs, shift_delta): one lane / past a 32-column tile / past a row tile with an uneven last
# slice; every TrainBackRow<T> (D 32 .. 128, 256, 384, 512); A + 1 below a tile, across 64, full
CASES = [(1, 18, 32, 0, 9, True, 0), (33, 84, 96, 1, 65, False, 0), (130, 512, 512, 2, 127, True, 0),
         (130, 18, 32, 2, 9, False, -2), (33, 18, 256, 1, 127, False, 0), (130, 84, 384, 1, 65, True, 0)]


def check_bound(net, x, dps, want, got):
    """|got - want| <= m c G_abs for every layer's dW and db; dps: the dp of every backward pass that was added up."""
    mags = [U.backward_np(net, x, dp, absolute=True) for dp in dps]
    for i in range(len(net.layers)):
        for which in (0, 1):
            mag = sum(m[which][i] for m in mags)
            err = np.abs(got[which][i] - want[which][i])
            bound = U.depth(net, i) * train.ERR * mag
            print(f"layer {i} {'dW db'.split()[which]}: worst err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3g}")
            assert np.all(err <= bound), (i, which)


def run_case(net, x, seed):
    dp = np.random.default_rng(seed).standard_normal((len(x), net.actions + 1))
    want = U.twin(net, x, dp)
    got = U.twin(net, x, dp, kernels=True, device="cuda")
    assert np.array_equal(got[0], want[0])
    assert all(g.any() for g in want[1])
    check_bound(net, x, [dp], want[1:], got[1:])
    return dp, got


@pytest.mark.parametrize("case", CASES, ids=str)
def test_forward_and_backward(case):
    rows, f, d, blocks, a, binary, delta = case
    net = Net.random((f,), a, d, blocks, seed=rows + d, shift_delta=delta)
    x = U.rows_of(f, rows, 3, binary)
    dp, got = run_case(net, x, seed=1)
    again = U.twin(net, x, dp, kernels=True, device="cuda")  # the same inputs: the same bits
    assert all(np.array_equal(a, b) for a, b in zip(got[1] + got[2], again[1] + again[2]))


def test_boundary_net():
    run_case(*U.crafted(), seed=2)


@pytest.mark.parametrize("kind", [0, 1], ids=["discrete", "box"])
def test_actor(kind):
    """`logp` and `value` make two forward passes and one backward: both through the kernels, added up."""
    h = 3
    space = dict(features=11, kind=kind, actions=h, obs_low=np.full(11, -1.0), obs_high=np.full(11, 1.0),
                 low=np.full(h if kind else 0, -1, np.float32), high=np.full(h if kind else 0, 1, np.float32))
    actor = Actor.random(space, hidden=64, blocks=1, seed=2)
    rng = np.random.default_rng(4)
    obs = torch.tensor(rng.uniform(-1, 1, (70, 11)))
    action = torch.tensor(rng.uniform(-1, 1, (70, h)) if kind else rng.integers(0, h, 70))
    ref, fast = actor.module(), actor.module(kernels=True).to("cuda")
    seen, plain = [], ref.net.integers
    ref.net.integers = lambda x: seen.append(plain(x)) or seen[-1].retain_grad() or seen[-1]
    (ref.logp(obs, action).sum() + ref.value(obs).to(torch.float64).sum()).backward()
    (fast.logp(obs.cuda(), action.cuda()).sum() + fast.value(obs.cuda()).to(torch.float64).sum()).backward()
    grads = lambda m: ([w.grad.cpu().numpy() for w in m.net.weights], [b.grad.cpu().numpy() for b in m.net.biases])
    x = ref.features(obs).detach().numpy().astype(np.uint8)
    assert len(seen) == 2 and grads(ref)[0][0].any()
    check_bound(actor.net, x, [p.grad.numpy() for p in seen], grads(ref), grads(fast))


def test_module_on_device():
    """Parameters left on the CPU are refused, not read; an input outside 0 .. 127 is what the CPU path makes of it;
    `release()` frees the handles and the next step makes its own."""
    net = Net.random((18,), 9, 32, 1, seed=4)
    with pytest.raises(ValueError, match="a parameter is on cpu"):
        net.module(kernels=True).integers(torch.zeros((2, 18), device="cuda"))
    odd = torch.tensor(np.random.default_rng(5).uniform(-40, 170, (9, 18)))
    m = net.module(kernels=True)
    want = m.integers(odd)
    assert torch.equal(m.to("cuda").integers(odd.cuda()).cpu(), want)
    assert train._handles
    train.release()
    assert not train._handles
    assert torch.equal(m.integers(odd.cuda()).cpu(), want)


def test_c_refusals():
    lib, dev = native.lib(), torch.device("cuda", 0)
    out = ctypes.c_void_p()
    with pytest.raises(ValueError, match="D = 48"):
        native.check(lib.epa_net_train_create(0, 18, 9, 48, 1, 64, ctypes.byref(out)))
    with pytest.raises(ValueError, match="rows = 1048577"):
        native.check(lib.epa_net_train_create(0, 18, 9, 32, 1, 2 ** 20 + 1, ctypes.byref(out)))
    native.check(lib.epa_net_train_create(0, 18, 9, 32, 0, 64, ctypes.byref(out)))
    try:
        w = [torch.ones((32, 18), dtype=torch.int8, device=dev), torch.ones((10, 32), dtype=torch.int8, device=dev)]
        b = [torch.zeros(32, dtype=torch.int32, device=dev), torch.zeros(10, dtype=torch.int32, device=dev)]
        dw, db = [torch.zeros(t.shape, device=dev) for t in w], [torch.zeros(t.shape, device=dev) for t in b]
        x, p = torch.ones((5, 18), dtype=torch.uint8, device=dev), torch.zeros((5, 10), dtype=torch.int32, device=dev)
        dp = torch.ones((5, 10), device=dev)
        ptr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        backward = lambda rows: native.check(lib.epa_net_train_backward_device(out, stream, rows, dp.data_ptr(), ptr(dw),
                                                                               ptr(db)))
        forward = lambda rows, shifts: native.check(lib.epa_net_train_forward_device(
            out, stream, rows, ptr(w), ptr(b), (ctypes.c_int32 * 2)(*shifts), x.data_ptr(), p.data_ptr()))
        with pytest.raises(ValueError, match="no forward"):
            backward(5)
        with pytest.raises(ValueError, match="rows = 65"):
            forward(65, (3, 0))
        with pytest.raises(ValueError, match="shift = 1"):
            forward(5, (3, 1))
        forward(5, (3, 0))
        with pytest.raises(ValueError, match="the last forward had 5"):
            backward(4)
        backward(5)
        torch.cuda.synchronize()
        assert torch.equal(p, torch.full((5, 10), 32 * ((18 + 4) >> 3), dtype=torch.int32, device=dev))
        assert torch.equal(db[1], torch.full((10,), 5.0, device=dev))
    finally:
        native.check(lib.epa_net_train_destroy(out))
