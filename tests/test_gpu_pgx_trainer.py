"""The PGX trainer on the device (csrc/pgx_trainer.hip, `net.trainer(...)`) against the float64 numpy restatements of
its contract (tests/pgx_trainer_util.py): loss, wiring, update and re-quantising, `fit`, and the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import pgx_net_util as NU
import pgx_train_util as TU
import pgx_trainer_util as U
from envpool_amd.core import native
from envpool_amd.core.device_pool import DevicePool
from envpool_amd.pgx import train, trainer as T
from envpool_amd.pgx.net import ConvNet, Net
from envpool_amd.python.envpool import Samples

pytestmark = pytest.mark.gpu
DENSE = lambda: Net.random((17,), 9, 32, 1, seed=3)
CONV = lambda: ConvNet.random((3, 3, 2), 9, 32, 1, 2, seed=4)


def arrays(tr, what, net):
    return [tr.read(what, i) for i in range(2 * len(net.layers))]


# (rows, A): one row; rows past a block; A + 1 just below, at and above a wave's 64 lanes
@pytest.mark.parametrize("rows,a", [(1, 9), (65, 63), (130, 64), (70, 127)])
def test_loss(rows, a):
    net = Net.random((18,), a, 32, 0, seed=rows)
    obs, mask, pi, z = U.batch(rows, 18, a, seed=a)
    tr = net.trainer(lr=0.0, value_weight=0.5, max_rows=rows)
    tr.step(obs, mask, pi, z)
    p = tr.read(T.P)
    assert np.array_equal(p, TU.forward_np(net, obs)[1])
    want, mag, pol, pol_mag, val = U.loss(p, mask, pi, z, net.scale_p, net.scale_v, 0.5)
    dp, stats = tr.read(T.DP), tr.stats()
    print(f"worst err / bound = {np.max(np.abs(dp - want) / np.maximum(U.LOSS_ERR * mag, 1e-300)):.3g}")
    assert np.all(np.abs(dp - want) <= U.LOSS_ERR * mag) and want[:, :a].any()
    assert stats.shape == (1, 4) and stats[0, 3] == rows
    assert abs(stats[0, 0] - pol) <= U.LOSS_ERR * pol_mag and abs(stats[0, 1] - val) <= U.LOSS_ERR * val
    tr.close()


@pytest.mark.parametrize("make", [DENSE, CONV], ids=["net", "conv"])
def test_wiring(make):
    net = make()
    obs, mask, pi, z = U.batch(40, net.inputs, 9, seed=1)
    tr = net.trainer(lr=0.0, max_rows=64)
    tr.step(obs, mask, pi, z)
    dev = torch.device("cuda", 0)
    conv = isinstance(net, ConvNet)
    sizes = net.obs_shape + (9, 32, 1, 2) if conv else (17, 9, 32, 1)
    h = train._Handle("conv" if conv else "net", 0, sizes, 64)
    wq = [torch.from_numpy(tr.read(T.QUANTISED, i)).to(dev) for i in range(len(net.layers))]
    bq = [torch.from_numpy(tr.read(T.QUANTISED, len(net.layers) + i)).to(dev) for i in range(len(net.layers))]
    p = train._forward(h, 0, sizes, [s for _, _, s in net.layers], torch.from_numpy(obs).to(dev), wq, bq)
    dp = torch.from_numpy(tr.read(T.DP)).to(dev)
    grads = [torch.empty(t.shape, dtype=torch.float32, device=dev) for t in wq + bq]
    native.check(h.call("backward_device")(h._h, ctypes.c_void_p(0), 40, dp.data_ptr(),
                                           train._pointers(grads[:len(wq)]), train._pointers(grads[len(wq):])))
    torch.cuda.synchronize()
    assert np.array_equal(p.cpu().numpy(), tr.read(T.P))
    for want, got in zip(grads, arrays(tr, T.GRADIENT, net)):
        assert np.array_equal(want.cpu().numpy(), got) and got.any()
    h.close(), tr.close()


@pytest.mark.parametrize("make", [DENSE, CONV], ids=["net", "conv"])
@pytest.mark.parametrize("optimizer,clipped", [("sgd", False), ("adam", False), ("sgd", True)])
def test_update(make, optimizer, clipped):
    net = make()
    n = len(net.layers)
    obs, mask, pi, z = U.batch(40, net.inputs, 9, seed=2)
    probe = net.trainer(lr=0.0, max_rows=64)  # the first gradient: what the step sizes are chosen by
    probe.step(obs, mask, pi, z)
    first, norm = arrays(probe, T.GRADIENT, net), probe.stats()[0, 2]
    probe.close()
    clip = norm / 2 if clipped else 0.0
    # the largest first change of a weight is 300 (adam: all about 30): past the clamp, smaller ones cross roundings
    lr = 30.0 if optimizer == "adam" else 300.0 / (max(np.abs(g).max() for g in first[:n]) * (0.5 if clipped else 1.0))
    top = max(np.abs(g).max() for g in first[:n])
    # (weight decay and adam's eps below the gradients, which are small: dp carries scale_p / rows)
    options = dict(optimizer=optimizer, lr=lr, momentum=0.9, weight_decay=1e-4 * top, clip=clip, eps=1e-6 * top)
    tr = net.trainer(max_rows=64, **options)
    rule = U.Rule([w for w, _, _ in net.layers] + [b for _, b, _ in net.layers], **options)
    for step in range(2):  # (the second step reads the state the first wrote)
        tr.step(obs, mask, pi, z)
        got_norm = rule.step(arrays(tr, T.GRADIENT, net))
        assert got_norm == tr.stats()[0, 2] and (not clipped or step > 0 or got_norm > clip)  # (the clip bites)
        for i in range(2 * n):
            assert np.array_equal(tr.read(T.MASTER, i), rule.master[i]), (step, i)
            assert np.array_equal(tr.read(T.STATE1, i), rule.s1[i]), (step, i)
            assert optimizer == "sgd" or np.array_equal(tr.read(T.STATE2, i), rule.s2[i]), (step, i)
            assert np.array_equal(tr.read(T.QUANTISED, i), rule.quantised(i, i < n)), (step, i)
    moved = [rule.quantised(i, True) != net.layers[i][0] for i in range(n)]
    assert any((np.abs(rule.master[i]) > 127.5).any() for i in range(n)) and any(m.any() for m in moved)
    tr.close()


def test_fit_is_step_on_the_hashed_rows():
    net = Net.random((3, 3, 2), 9, 32, 1, seed=6)
    obs, mask, pi, z = U.batch(50, 18, 9, seed=3)
    s = Samples(obs.reshape(50, 3, 3, 2).astype(bool), mask.astype(bool), pi, z, None, None, None)
    probe = net.trainer(lr=0.0, max_rows=50)
    probe.step(obs, mask, pi, z)
    lr = 20.0 / max(np.abs(probe.read(T.GRADIENT, i)).max() for i in range(len(net.layers)))  # weights move by tens
    probe.close()
    options = dict(lr=lr, momentum=0.5, seed=5, max_rows=33)
    a, b, c = (net.trainer(**options) for _ in range(3))
    a.fit(s, batch=33, steps=3)
    for t in range(3):
        rows = [U.index(5, t, j, 50) for j in range(33)]
        b.step(obs[rows], mask[rows], pi[rows], z[rows])
    c.fit(s, batch=33, steps=2)
    c.fit(s, batch=33, steps=1)
    assert a.stats().shape == (3, 4) and c.stats().shape == (1, 4)
    masters = arrays(a, T.MASTER, net)
    assert any((m != np.rint(m)).any() for m in masters)
    for other in (b, c):
        assert all(np.array_equal(x, y) for x, y in zip(masters, arrays(other, T.MASTER, net)))
    # tr.net() is the twin of the final masters, and evaluates as such
    n = len(net.layers)
    layers = [(np.clip(np.rint(masters[i]), -127, 127).astype(np.int8),
               np.clip(np.rint(masters[n + i]), -2 ** 30, 2 ** 30).astype(np.int32), net.layers[i][2]) for i in range(n)]
    new = a.net()
    assert any((l[0] != o[0]).any() for l, o in zip(layers, net.layers))
    pool = DevicePool("TicTacToe", 8, seed=1)
    status = np.zeros(50, np.uint8)
    want = NU.restate(layers, 1, net.scale_p, net.scale_v, obs, mask, status, True)
    got = new.bind(pool, priors=True)(obs, mask, status)
    assert all(np.array_equal(x, y) for x, y in zip(got, want))
    [t.close() for t in (a, b, c, new)]


BAD_OPTIONS = [dict(optimizer="lion"), dict(lr=-1.0), dict(momentum=float("nan")), dict(betas=(0.9, float("inf"))),
               dict(betas=(-0.1, 0.9)), dict(eps=-1e-8), dict(weight_decay=-1.0), dict(value_weight=float("inf")),
               dict(clip=-1.0), dict(max_rows=0)]


@pytest.mark.parametrize("bad", BAD_OPTIONS + ["rows", "batch", "count", "steps", "null", "blob"], ids=str)
def test_refusals(bad):
    net, lib = DENSE(), native.lib()
    if isinstance(bad, dict):
        with pytest.raises(ValueError):
            net.trainer(**bad)
        o = native.TrainerOptions(2 if "optimizer" in bad else 0, 0, *[
            dict(lr=bad.get("lr", 1.0), momentum=bad.get("momentum", 0.9), beta1=bad.get("betas", (0.9, 0.9))[0],
                 beta2=bad.get("betas", (0.9, 0.9))[1], eps=bad.get("eps", 1e-8), wd=bad.get("weight_decay", 0.0),
                 vw=bad.get("value_weight", 1.0), clip=bad.get("clip", 0.0))[k]
            for k in ("lr", "momentum", "beta1", "beta2", "eps", "wd", "vw", "clip")], 0)
        blob, out = net.blob(), ctypes.c_void_p()
        assert lib.epa_trainer_create(0, blob.ctypes.data, blob.nbytes, ctypes.byref(o), bad.get("max_rows", 64),
                                      ctypes.byref(out)) == native.EPA_ERR_INVALID
        return
    tr = net.trainer(max_rows=8)
    obs, mask, pi, z = U.batch(9, 17, 9, seed=1)
    s = Samples(obs, mask, pi, z, None, None, None)
    ptrs = (ctypes.c_void_p * 4)(1, 1, 1, 1)  # (refused before anything reads them)
    with pytest.raises(ValueError):
        if bad == "rows":
            tr.step(obs, mask, pi, z)
        elif bad == "batch":
            tr.fit(s, batch=9)
        elif bad == "steps":
            tr.fit(s, batch=8, steps=0)
        elif bad == "count":
            native.check(lib.epa_trainer_fit_device(tr._h, None, ptrs, 0, 8, 1))
        elif bad == "null":
            native.check(lib.epa_trainer_step_device(tr._h, None, 8, None, 1, 1, 1))
        else:
            blob, out, o = net.blob(), ctypes.c_void_p(), native.TrainerOptions(0, 0, 1.0, 0.9, 0.9, 0.999, 1e-8, 0, 1, 0, 0)
            native.check(lib.epa_trainer_create(0, blob.ctypes.data, blob.nbytes - 4, ctypes.byref(o), 8,
                                                ctypes.byref(out)))
    tr.close()
