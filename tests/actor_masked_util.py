"""The masked head of the rollout actor (kind 2 of csrc/actor.hip.h and ppo_trainer.hip.h) restated in numpy,
independently of the headers: the legal words, the sample in float32 steps (the contract fixes its bits) and the loss in
float64 with the magnitudes kPpoErr multiplies, both over the legal set only."""
import numpy as np

import actor_util as au
from pgx_gumbel_util import exp_
from pgx_selfplay_util import gumbel_log, noise_of

F = np.float32


def masks(rng, rows, h):
    """bool [rows, H] of density 1/2, then the crafted rows: one legal action, only j = H - 1, all, none."""
    m = rng.random((rows, h)) < 0.5
    m[0], m[1], m[2], m[3] = False, False, True, False
    m[0, rng.integers(h)] = m[1, h - 1] = True
    return m


def legal_of(mask):
    """bool [rows, H] of raw mask rows: != 0, and a row without any is all legal."""
    ok = np.asarray(mask).reshape(len(mask), -1) != 0
    return ok | ~ok.any(axis=1, keepdims=True)


def words(mask):
    """uint32 [rows, 4]: bit j in word j // 32, bits H .. 127 clear; a row without a legal action is all ones."""
    ok = np.asarray(mask).reshape(len(mask), -1) != 0
    bits = np.zeros((len(ok), 128), np.uint8)
    bits[:, :ok.shape[1]] = ok
    bits[~ok.any(axis=1)] = 1
    return np.packbits(bits, axis=1, bitorder="little").view("<u4").astype(np.uint32)


def sample(p, legal, scale_p, scale_v, seed, env_ids, step, deterministic):
    """(flat action int32 [rows], logp, value float32 [rows]) from the head's integers p [rows, H + 1]."""
    p = np.asarray(p, np.int32)
    h = p.shape[1] - 1
    logit = p[:, :h].astype(F) * F(scale_p)
    score = logit if deterministic else logit + noise_of(au.uniforms(au.key(seed, env_ids, step), h))
    action = np.where(legal, score, -np.inf).argmax(axis=1).astype(np.int32)  # the first maximum: the lowest legal j
    top = np.where(legal, logit, -np.inf).max(axis=1).astype(F)
    total = np.zeros(len(p), F)
    for j in range(h):  # ascending j, the legal ones
        total = np.where(legal[:, j], total + exp_(logit[:, j] - top), total).astype(F)
    logp = (logit[np.arange(len(p)), action] - top) - gumbel_log(total)
    assert logp.dtype == F
    return action, logp, p[:, h].astype(F) * F(scale_v)


def loss(p, legal, action, logp, adv, ret, mask, scale_p, scale_v, clip_ratio, value_weight, entropy_weight):
    """ppo_trainer_util.loss's discrete branch with every sum, maximum and magnitude over the legal set: float64 dp, mag
    [n, H + 1] (0 at an illegal j), stat, stat_mag [n, 5], lp, d, active, near [n]."""
    n, h = p.shape[0], p.shape[1] - 1
    sp, sv, vw, nf = float(F(scale_p)), float(F(scale_v)), float(F(value_weight)), float(F(n))
    lo, hi, ew = float(F(1) - F(clip_ratio)), float(F(1) + F(clip_ratio)), float(F(entropy_weight) / F(n))
    l = (p[:, :h].astype(F) * F(scale_p)).astype(np.float64)
    v = (p[:, h].astype(F) * F(scale_v)).astype(np.float64)
    adv, ret, logp = (x.astype(np.float64) for x in (adv, ret, logp))
    x = l - np.where(legal, l, -np.inf).max(axis=1, keepdims=True)
    e = np.where(legal, np.exp(np.clip(x, -87.0, 0.0)), 0.0)
    s = e.sum(axis=1, keepdims=True)
    q, lq = e / s, np.where(legal, x - np.log(s), 0.0)
    hn = -(q * lq).sum(axis=1)
    lp = (x - np.log(s))[np.arange(n), action]
    w = 1.0 + np.where(legal, np.abs(x) + np.abs(np.log(s)), 0.0).max(axis=1) / 128.0
    d = np.clip(lp - logp, -20.0, 20.0)
    r = np.exp(d)
    rc = np.clip(r, lo, hi)
    active = r * adv <= rc * adv
    g = np.where(active, -(adv * r) / nf, 0.0)[:, None]
    hit = np.arange(h)[None, :] == np.asarray(action)[:, None]
    dp, mag = np.zeros(p.shape), np.zeros(p.shape)
    dp[:, :h] = np.where(legal, sp * (g * (hit - q) + ew * q * (lq + hn[:, None])), 0.0)
    mag[:, :h] = np.where(legal, sp * w[:, None] * (np.abs(g) * (hit + q) + ew * q * (np.abs(lq) + hn[:, None] + 1.0)), 0.0)
    dp[:, h] = 2.0 * vw * sv * (v - ret) / nf
    mag[:, h] = np.abs(dp[:, h])
    val = vw * (v - ret) ** 2
    stat = np.stack([-np.minimum(r * adv, rc * adv), val, hn, (r - 1.0) - d, (r != rc).astype(np.float64)], axis=1)
    stat_mag = np.stack([w * np.abs(adv) * np.maximum(r, rc), val, w * (hn + 1.0), w * (r + 1.0), np.zeros(n)], axis=1)
    near = np.minimum(np.abs(r - lo), np.abs(r - hi)) <= 4 * 1.9e-5 * w * r
    z0 = (mask != 0)[:, None].astype(np.float64)
    return dict(dp=dp * z0, mag=mag * z0, stat=stat * z0, stat_mag=stat_mag * z0, lp=lp, d=d, active=active, near=near)
