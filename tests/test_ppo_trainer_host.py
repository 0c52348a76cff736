"""The PPO trainer's contract without a GPU: csrc/ppo_trainer.hip.h built by g++ (cpu_harness/ppo_trainer_host.cpp)
against the float64 restatement (ppo_trainer_util.py): the loss of both heads within kPpoErr; the permutation, the
advantage tree, the sigma sum and floor bit for bit; and the refusals of `actor.trainer(...)` that need no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ppo_trainer_util as U
from envpool_amd.actor import Actor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"]
SRC = os.path.join(ROOT, "tests", "cpu_harness", "ppo_trainer_host.cpp")
ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
SCALE_P, SCALE_V, CLIP, VW, EW = 1.0 / 3000.0, 1.0 / 50000.0, 0.2, 0.5, 0.01


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ppo_trainer") / "libppotrainerhost.so")
    subprocess.run(FLAGS + ["-shared", "-fPIC", SRC, "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.ppo_err.restype = ctypes.c_double
    L.ppo_permute.restype = ctypes.c_uint32
    L.ppo_permute.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    L.ppo_adv_normalize.restype = L.ppo_sigma_of.restype = ctypes.c_float
    L.ppo_adv_normalize.argtypes = [ctypes.c_float, ctypes.c_double, ctypes.c_double]
    L.ppo_sigma_of.argtypes = [ctypes.c_double]
    L.ppo_loss_discrete.argtypes = [ctypes.c_int] * 2 + [ctypes.c_void_p] * 6 + [ctypes.c_float] * 5 + [ctypes.c_void_p] * 2
    L.ppo_loss_box.argtypes = [ctypes.c_int] * 2 + [ctypes.c_void_p] * 7 + [ctypes.c_float] * 5 + [ctypes.c_void_p] * 3
    return L


@pytest.mark.parametrize("rows", [1, 65])
@pytest.mark.parametrize("kind,h", [(0, 2), (0, 63), (0, 127), (1, 1), (1, 6), (1, 17)])
def test_loss_within_the_derived_bound(lib, kind, h, rows):
    assert lib.ppo_err() == U.ERR
    rng = np.random.default_rng(100 * h + rows)
    top = 60000 if kind == U.DISCRETE else 3000  # logits to +-20; means to +-1, inside the action bounds
    p = rng.integers(-top, top, size=(rows, h + 1)).astype(np.int32)
    sigma = rng.uniform(0.05, 1.5, h).astype(np.float32) if kind == U.BOX else None
    action, logp, adv, ret, mask = U.batch(kind, p, h, SCALE_P, sigma)
    dp, stat = np.zeros((rows, h + 1), np.float32), np.zeros((rows, 5), np.float32)
    dsigma = np.zeros((rows, h), np.float32)
    if kind == U.DISCRETE:
        lib.ppo_loss_discrete(rows, h, ptr(p), ptr(action), ptr(logp), ptr(adv), ptr(ret), ptr(mask), SCALE_P, SCALE_V,
                              CLIP, VW, EW, ptr(dp), ptr(stat))
    else:
        lib.ppo_loss_box(rows, h, ptr(p), ptr(action), ptr(sigma), ptr(logp), ptr(adv), ptr(ret), ptr(mask), SCALE_P,
                         SCALE_V, CLIP, VW, EW, ptr(dp), ptr(stat), ptr(dsigma))
    want = U.loss(kind, p, action, logp, adv, ret, mask, SCALE_P, SCALE_V, CLIP, VW, EW, sigma)
    if rows > 1:
        U.check_draw(kind, want, mask, action)
        assert not dp[1].any() and not stat[1].any() and not dsigma[1].any()  # the masked row
    checks = [U.within(dp, want["dp"], want["mag"]), U.within(stat, want["stat"], want["stat_mag"])]
    if kind == U.BOX:
        checks.append(U.within(dsigma, want["dsigma"], want["dsigma_mag"]))
        total = np.zeros(h, np.float32)
        lib.ppo_sigma_sum(ptr(dsigma), ptr(mask), rows, h, ptr(total))
        blocks = [dsigma[r:r + U.LOSS_ROWS][mask[r:r + U.LOSS_ROWS] != 0].astype(np.float64)
                  for r in range(0, rows, U.LOSS_ROWS)]
        by_hand = np.zeros(h)
        for b in blocks:
            s = np.zeros(h)
            for row in b:
                s = s + row
            by_hand = by_hand + s
        assert np.array_equal(total, by_hand.astype(np.float32))
    print(f"worst err / bound = {max(w for _, w in checks):.3g}")
    assert all(ok for ok, _ in checks) and want["dp"].any()


@pytest.mark.parametrize("n", [1, 2, 5, 64, 65, 1000])
def test_permute_is_a_bijection_and_differs_between_epochs(lib, n):
    images = [[lib.ppo_permute(7, epoch, j, n) for j in range(n)] for epoch in (0, 1)]
    for epoch, image in enumerate(images):
        assert sorted(image) == list(range(n))
        assert image == [U.permute(7, epoch, j, n) for j in range(n)]
    assert n < 5 or images[0] != images[1]


@pytest.mark.parametrize("n", [1, 240, 1024, 2500])
def test_advantage_tree(lib, n):
    rng = np.random.default_rng(n)
    adv = (rng.standard_normal(n) * 3 + 1).astype(np.float32)
    mask = (rng.random(n) < 0.8).astype(np.uint8)
    mask[0] = 1
    out = np.zeros(3)
    lib.ppo_adv_stats(ptr(adv), ptr(mask), n, ptr(out))
    cnt, mean, std = U.adv_stats(adv, mask)
    assert (out[0], out[1], out[2]) == (cnt, mean, std) and cnt == mask.sum()
    got = np.array([lib.ppo_adv_normalize(float(a), mean, std) for a in adv[:16]], np.float32)
    assert np.array_equal(got, U.adv_normalize(adv[:16], mean, std))
    lib.ppo_adv_stats(ptr(adv), ptr(np.zeros(n, np.uint8)), n, ptr(out))
    assert not out.any()


@pytest.mark.parametrize("master,want", [(0.5, 0.5), (U.SIGMA_MIN, U.SIGMA_MIN), (1e-4, U.SIGMA_MIN), (-3.0, U.SIGMA_MIN),
                                         (1.0 + 2.0 ** -30, 1.0)])
def test_sigma_floor(lib, master, want):
    assert lib.ppo_sigma_of(master) == np.float32(want)


@pytest.mark.parametrize("bad", [dict(optimizer="lion"), dict(lr=-1.0), dict(clip_ratio=float("nan")),
                                 dict(entropy_weight=-0.1), dict(betas=(0.9, float("inf"))), dict(max_rows=0),
                                 dict(max_rows=(1 << 22) + 1), dict(normalize_adv=1), dict(train_sigma="yes")], ids=str)
def test_refusals_without_a_device(bad):
    actor = Actor.random(dict(features=4, kind=0, actions=2, low=np.zeros(0, np.float32), high=np.zeros(0, np.float32),
                              obs_low=np.full(4, -1.0), obs_high=np.full(4, 1.0)), hidden=32, blocks=0)
    with pytest.raises(ValueError):
        actor.trainer(**bad)
