"""Shared by the training tests of the PGX convolutional network (test_pgx_conv_train_host.py,
test_gpu_pgx_conv_train.py): the reference -- the float64 twin `ConvNet.module()` with autograd on the CPU --, a numpy
restatement of the same backward pass that can also run over magnitudes (G_abs of the error bound), and the crafted
boundary net."""
import numpy as np
import torch

from envpool_amd.pgx.net import ConvNet


def boards_of(shape, rows, seed=3):
    """Input bytes [rows, H, W, C]: 0 / 1 of density 1/4."""
    return (np.random.default_rng(seed).random((rows,) + tuple(shape)) < 0.25).astype(np.uint8)


def twin(net, x, dp, kernels=False, device="cpu"):
    """(p, [dW], [db]) of `net`'s module for the loss SUM p * dp, everything as float64 numpy."""
    m = net.module(kernels=kernels).to(device)
    p = m.integers(torch.tensor(x.astype(np.float64), device=device))
    (p * torch.tensor(dp, device=device)).sum().backward()
    return (p.detach().cpu().numpy(), [w.grad.cpu().numpy().astype(np.float64) for w in m.weights],
            [b.grad.cpu().numpy().astype(np.float64) for b in m.biases])


def _pad(a):
    return np.pad(a, ((0, 0), (1, 1), (1, 1), (0, 0)))


def _conv(a, w):
    """a [R, H, W, K], w [N, 3, 3, K] -> [R, H, W, N], zero padding."""
    ap, (h, wd) = _pad(a), a.shape[1:3]
    return sum(ap[:, dy:dy + h, dx:dx + wd] @ w[:, dy, dx].T for dy in range(3) for dx in range(3))


def forward_np(net, x):
    """The values before the clamps: j = 0 .. 2 L (int64 [rows, H, W, D] each), the reduce layer's, and p."""
    rs = lambda z, s: (z + ((1 << (s - 1)) if s else 0)) >> s
    w = [l[0].astype(np.int64) for l in net.layers]
    lay = lambda i, a: rs((_conv(a, w[i]) if w[i].ndim == 4 else a @ w[i].T) + net.layers[i][1], net.layers[i][2])
    pre = [lay(0, x.astype(np.int64))]
    h = np.clip(pre[0], 0, 127)
    for l in range(net.blocks):
        pre.append(lay(1 + 2 * l, h))
        pre.append(lay(2 + 2 * l, np.clip(pre[-1], 0, 127)) + h)
        h = np.clip(pre[-1], 0, 127)
    pre_g = lay(2 * net.blocks + 1, h)
    return pre, pre_g, lay(2 * net.blocks + 2, np.clip(pre_g, 0, 127).reshape(len(x), -1))


def backward_np(net, x, dp, absolute=False):
    """([dW], [db]) by the contract's rules in float64; `absolute`: over |W| and |dp| with the same masks."""
    pre, pre_g, _ = forward_np(net, x)
    act = [np.clip(q, 0, 127).astype(np.float64) for q in pre]
    keep = [((q >= 0) & (q <= 127)).astype(np.float64) for q in pre]
    wt = [np.abs(w.astype(np.float64)) if absolute else w.astype(np.float64) for w, _, _ in net.layers]
    sc = [2.0 ** -s for _, _, s in net.layers]
    n, (rows, h, wd) = len(net.layers), x.shape[:3]
    dw, db = [None] * n, [None] * n

    def reduce(i, dz):  # a 3x3 layer
        ap = _pad(x.astype(np.float64) if i == 0 else act[i - 1])
        dw[i] = np.stack([np.stack([np.einsum("ryxn,ryxc->nc", dz, ap[:, dy:dy + h, dx:dx + wd]) for dx in range(3)],
                                   axis=1) for dy in range(3)], axis=1)
        db[i] = dz.sum(axis=(0, 1, 2))

    def below(i, dz):
        zp = _pad(dz)
        return sum(zp[:, 2 - dy:2 - dy + h, 2 - dx:2 - dx + wd] @ wt[i][:, dy, dx] for dy in range(3) for dx in range(3))

    dz = np.abs(dp) if absolute else dp
    g = np.clip(pre_g, 0, 127).astype(np.float64)
    dw[n - 1], db[n - 1] = dz.T @ g.reshape(rows, -1), dz.sum(axis=0)
    dr = (dz @ wt[n - 1]).reshape(pre_g.shape) * ((pre_g >= 0) & (pre_g <= 127)) * sc[n - 2]
    dw[n - 2], db[n - 2] = np.einsum("ryxq,ryxc->qc", dr, act[-1]), dr.sum(axis=(0, 1, 2))
    a = (dr @ wt[n - 2]) * keep[-1] * sc[n - 3]
    for l in range(net.blocks - 1, -1, -1):
        reduce(2 + 2 * l, a)
        b = below(2 + 2 * l, a) * keep[1 + 2 * l] * sc[1 + 2 * l]
        reduce(1 + 2 * l, b)
        a = (below(1 + 2 * l, b) + a / sc[2 + 2 * l]) * keep[2 * l] * sc[2 * l]
    reduce(0, a)
    return dw, db


def crafted():
    """(net, x): a 2x2 board, one block of centre-tap identities whose biases put the values before both of the block's
    clamps and before the reduce layer's at exactly -1, 0, 127 and 128 in square 0 of row 0 (channels 0 .. 3: t;
    4 .. 7: h_new; 8 .. 11 through the four planes: g), beside ordinary squares and rows."""
    d, planes = 32, 4
    eye = np.zeros((d, 3, 3, d), np.int8)
    eye[:, 1, 1, :] = np.eye(d, dtype=np.int8)
    b1, b2, br = np.zeros(d, np.int32), np.zeros(d, np.int32), np.array([-1, 0, 7, 8], np.int32)
    b1[[0, 3]] = -1, 1
    b2[2:4] = -127  # (h_new of channels 2 and 3 stays at 127: their t's gradient is not masked above)
    b2[4:8] = -1, 0, 7, 8
    wr = np.zeros((planes, d), np.int8)
    wr[np.arange(planes), 8 + np.arange(planes)] = 1
    head = np.random.default_rng(5).integers(-127, 128, size=(4, 4 * planes)).astype(np.int8)
    zero = np.zeros(d, np.int32)
    net = ConvNet((2, 2, d), 3, d, 1, planes, [(eye, zero, 0), (eye, b1, 0), (eye, b2, 0), (wr, br, 0),
                                               (head, np.zeros(4, np.int32), 0)], 1e-3, 1e-3)
    x = np.random.default_rng(9).integers(0, 64, size=(3, 2, 2, d)).astype(np.uint8)
    x[0, 0, 0, :12] = 0, 0, 127, 127, 0, 0, 60, 60, 0, 0, 60, 60
    pre, pre_g, _ = forward_np(net, x)
    assert pre[1][0, 0, 0, :4].tolist() == [-1, 0, 127, 128] and pre[2][0, 0, 0, 4:8].tolist() == [-1, 0, 127, 128]
    assert pre_g[0, 0, 0].tolist() == [-1, 0, 127, 128]
    return net, x


def depth(net, i):
    """The layers between layer i and the output, inclusive: the m of the bound m c G_abs."""
    return len(net.layers) - i
