"""Shared by the training tests of the PGX built-in network (test_pgx_train_host.py, test_gpu_pgx_train.py): the
reference -- the float64 twin `Net.module()` with autograd on the CPU --, a numpy restatement of the same backward pass
that can also run over magnitudes (G_abs of the error bound), and the crafted boundary net."""
import numpy as np
import torch

from envpool_amd.pgx.net import Net


def rows_of(f, rows, seed, binary):
    """Input bytes: 0 / 1 of density 1/4, or spread over 0 .. 127."""
    rng = np.random.default_rng(seed)
    if binary:
        return (rng.random((rows, f)) < 0.25).astype(np.uint8)
    return rng.integers(0, 128, size=(rows, f)).astype(np.uint8)


def twin(net, x, dp, kernels=False, device="cpu"):
    """(p, [dW], [db]) of `net`'s module for the loss SUM p * dp, everything as float64 numpy."""
    m = net.module(kernels=kernels).to(device)
    p = m.integers(torch.tensor(x.astype(np.float64), device=device))
    (p * torch.tensor(dp, device=device)).sum().backward()
    return (p.detach().cpu().numpy(), [w.grad.cpu().numpy().astype(np.float64) for w in m.weights],
            [b.grad.cpu().numpy().astype(np.float64) for b in m.biases])


def forward_np(net, x):
    """The values before the clamps, j = 0 .. 2 L (int64 [rows, D] each), and p."""
    rs = lambda z, s: (z + ((1 << (s - 1)) if s else 0)) >> s
    lay = lambda i, a: rs(a @ net.layers[i][0].astype(np.int64).T + net.layers[i][1], net.layers[i][2])
    pre = [lay(0, x.astype(np.int64))]
    h = np.clip(pre[0], 0, 127)
    for l in range(net.blocks):
        pre.append(lay(1 + 2 * l, h))
        pre.append(lay(2 + 2 * l, np.clip(pre[-1], 0, 127)) + h)
        h = np.clip(pre[-1], 0, 127)
    return pre, lay(2 * net.blocks + 1, h)


def backward_np(net, x, dp, absolute=False):
    """([dW], [db]) by the contract's rules in float64; `absolute`: over |W| and |dp| with the same masks."""
    pre, _ = forward_np(net, x)
    act = [np.clip(q, 0, 127).astype(np.float64) for q in pre]
    keep = [((q >= 0) & (q <= 127)).astype(np.float64) for q in pre]
    wt = [np.abs(w.astype(np.float64)) if absolute else w.astype(np.float64) for w, _, _ in net.layers]
    sc = [2.0 ** -s for _, _, s in net.layers]
    n = len(net.layers)
    dw, db = [None] * n, [None] * n

    def reduce(i, dz):
        dw[i], db[i] = dz.T @ (x.astype(np.float64) if i == 0 else act[i - 1]), dz.sum(axis=0)

    dz = np.abs(dp) if absolute else dp
    reduce(n - 1, dz)
    a = (dz @ wt[n - 1]) * keep[n - 2] * sc[n - 2]
    for l in range(net.blocks - 1, -1, -1):
        reduce(2 + 2 * l, a)
        b = (a @ wt[2 + 2 * l]) * keep[1 + 2 * l] * sc[1 + 2 * l]
        reduce(1 + 2 * l, b)
        a = (b @ wt[1 + 2 * l] + a / sc[2 + 2 * l]) * keep[2 * l] * sc[2 * l]
    reduce(0, a)
    return dw, db


def crafted():
    """(net, x): one block of identities whose biases put the values before both of the block's clamps at exactly
    -1, 0, 127 and 128 in row 0 (neurons 0 .. 3: t; neurons 4 .. 7: h_new), beside two ordinary rows."""
    d = 32
    eye = np.eye(d, dtype=np.int8)
    b1, b2 = np.zeros(d, np.int32), np.zeros(d, np.int32)
    b1[[0, 3]] = -1, 1
    b2[2:4] = -127  # (h_new of neurons 2 and 3 stays at 127: their t's gradient is not masked above)
    b2[4:8] = -1, 0, 7, 8
    head = np.random.default_rng(5).integers(-127, 128, size=(4, d)).astype(np.int8)
    net = Net((d,), 3, d, 1, [(eye, np.zeros(d, np.int32), 0), (eye, b1, 0), (eye, b2, 0),
                              (head, np.zeros(4, np.int32), 0)], 1e-3, 1e-3)
    x = rows_of(d, 3, 9, False)
    x[0, :8] = 0, 0, 127, 127, 0, 0, 60, 60
    pre, _ = forward_np(net, x)
    assert pre[1][0, :4].tolist() == [-1, 0, 127, 128] and pre[2][0, 4:8].tolist() == [-1, 0, 127, 128]
    return net, x


def depth(net, i):
    """The layers between layer i and the output, inclusive: the m of the bound m c G_abs."""
    return len(net.layers) - i
