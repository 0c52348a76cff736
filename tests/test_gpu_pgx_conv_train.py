"""Training kernels of the PGX convolutional network on the device (csrc/pgx_conv_train.hip) against the float64 twin
`ConvNet.module()` with autograd on the CPU: the forward integers exactly, every gradient within m c_conv G_abs (the
contract header derives c_conv; G_abs is the same backward pass over |W|, |dp| and the same masks; m the layers up to
the output), at the shapes where the tiling can go wrong; the crafted boundary net; bit-identical repeats; the module
on the device; and the C-level refusals."""
import ctypes

import numpy as np
import pytest
import torch

import pgx_conv_train_util as U
from envpool_amd.core import native
from envpool_amd.pgx import train
from envpool_amd.pgx.net import ConvNet

pytestmark = pytest.mark.gpu
# (rows, H, W, C, D, L, P, A, shift_delta, net seed): one board, H != W, L = 0 / boards across column tiles, a partial
# group, several uneven reduction slices, H W P = 45 / three channel tiles, A + 1 across 32 / Othello, A + 1 across 64 /
# the widest D, C and P, a small G / Hex / a 1x1 board, 70 boards in one chunk
CASES = [(1, 3, 5, 3, 32, 0, 3, 9, 0, 0), (33, 3, 5, 3, 64, 1, 3, 9, -1, 0), (9, 4, 4, 2, 96, 1, 2, 40, 0, 105),
         (3, 8, 8, 2, 64, 2, 4, 64, 0, 0), (40, 2, 3, 32, 256, 1, 32, 127, 0, 296), (2, 11, 11, 3, 32, 1, 4, 121, 0, 34),
         (70, 1, 1, 2, 32, 1, 2, 3, 0, 0)]


def run_case(net, x, seed):
    dp = np.random.default_rng(seed).standard_normal((len(x), net.actions + 1))
    want = U.twin(net, x, dp)
    got = U.twin(net, x, dp, kernels=True, device="cuda")
    assert np.array_equal(got[0], want[0])
    assert all(g.any() for g in want[1] + want[2])
    mag = U.backward_np(net, x, dp, absolute=True)
    for i in range(len(net.layers)):
        for which in (0, 1):
            err = np.abs(got[1 + which][i] - want[1 + which][i])
            bound = U.depth(net, i) * train.CONV_ERR * mag[which][i]
            print(f"layer {i} {'dW db'.split()[which]}: worst err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3g}")
            assert np.all(err <= bound), (i, which)
    return dp, got


@pytest.mark.parametrize("case", CASES, ids=str)
def test_forward_and_backward(case):
    rows, h, w, c, d, blocks, planes, a, delta, seed = case
    net = ConvNet.random((h, w, c), a, d, blocks, planes, seed=seed, shift_delta=delta)
    x = U.boards_of((h, w, c), rows)
    dp, got = run_case(net, x, seed=1)
    again = U.twin(net, x, dp, kernels=True, device="cuda")  # the same inputs: the same bits
    assert all(np.array_equal(a, b) for a, b in zip(got[1] + got[2], again[1] + again[2]))


def test_boundary_net():
    run_case(*U.crafted(), seed=2)


def test_module_on_device():
    """Parameters left on the CPU are refused, not read; an input outside 0 .. 127 is what the CPU path makes of it;
    `release()` frees the handles and the next step makes its own."""
    net = ConvNet.random((3, 3, 2), 9, 32, 1, 2, seed=4)
    with pytest.raises(ValueError, match="a parameter is on cpu"):
        net.module(kernels=True).integers(torch.zeros((2, 3, 3, 2), device="cuda"))
    odd = torch.tensor(np.random.default_rng(5).uniform(-40, 170, (9, 3, 3, 2)))
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
        native.check(lib.epa_conv_train_create(0, 3, 3, 2, 9, 48, 1, 2, 64, ctypes.byref(out)))
    with pytest.raises(ValueError, match="rows = 466034"):
        native.check(lib.epa_conv_train_create(0, 3, 3, 2, 9, 32, 1, 2, 466034, ctypes.byref(out)))
    native.check(lib.epa_conv_train_create(0, 3, 3, 2, 9, 32, 0, 2, 64, ctypes.byref(out)))
    try:
        shapes = [(32, 3, 3, 2), (2, 32), (10, 18)]
        w = [torch.ones(s, dtype=torch.int8, device=dev) for s in shapes]
        b = [torch.zeros(s[0], dtype=torch.int32, device=dev) for s in shapes]
        dw, db = [torch.zeros(t.shape, device=dev) for t in w], [torch.zeros(t.shape, device=dev) for t in b]
        x = torch.ones((5, 3, 3, 2), dtype=torch.uint8, device=dev)
        p, dp = torch.zeros((5, 10), dtype=torch.int32, device=dev), torch.ones((5, 10), device=dev)
        ptr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        backward = lambda rows: native.check(lib.epa_conv_train_backward_device(out, stream, rows, dp.data_ptr(),
                                                                                ptr(dw), ptr(db)))
        forward = lambda rows, shifts: native.check(lib.epa_conv_train_forward_device(
            out, stream, rows, ptr(w), ptr(b), (ctypes.c_int32 * 3)(*shifts), x.data_ptr(), p.data_ptr()))
        with pytest.raises(ValueError, match="no forward"):
            backward(5)
        with pytest.raises(ValueError, match="rows = 65"):
            forward(65, (0, 0, 0))
        with pytest.raises(ValueError, match="shift = 1"):
            forward(5, (0, 0, 1))
        forward(5, (0, 3, 0))
        with pytest.raises(ValueError, match="the last forward had 5"):
            backward(4)
        backward(5)
        torch.cuda.synchronize()
        # the centre square sees 18 ones, an edge 12, a corner 8 in each of 32 channels; g = rs(32 h, 3) in both planes
        g = torch.tensor([8, 12, 8, 12, 18, 12, 8, 12, 8]) * 4
        assert torch.equal(p.cpu(), torch.full((5, 10), int(2 * g.sum()), dtype=torch.int32))
        assert torch.equal(db[2], torch.full((10,), 5.0, device=dev))
    finally:
        native.check(lib.epa_conv_train_destroy(out))
