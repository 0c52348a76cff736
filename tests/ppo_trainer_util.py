"""Shared by the PPO trainer tests: numpy float64 restatements of the contract csrc/ppo_trainer.hip.h -- the loss of
both heads with the magnitudes kPpoErr multiplies, the permutation, the advantage tree -- and the minibatch every loss
test uses.  Norm and update rule are pgx_trainer_util's."""
import numpy as np

from pgx_trainer_util import M64, Rule, mix, norm  # noqa: F401  (the update tests take them from here)

ERR = 2.0 ** -14        # kPpoErr
LOSS_ROWS = 32          # kPpoLossRows
ADV_CHUNK = 1024        # kPpoAdvChunk
SIGMA_MIN = 2.0 ** -10  # kPpoSigmaMin
F32 = np.float32
C = float(F32(0.9189385))
K = float(F32(0.5) + F32(0.9189385))
DISCRETE, BOX = 0, 1


def permute(seed, epoch, j, n):
    b = 1
    while b < 16 and (1 << (2 * b)) < n:
        b += 1
    half, x = (1 << b) - 1, j
    while True:
        left, right = x >> b, x & half
        for rnd in range(4):
            f = mix(seed ^ mix((epoch << 32) | (rnd << 16) | right))
            left, right = right, left ^ (f & half)
        x = (left << b) | right
        if x < n:
            return x


def adv_stats(adv, mask):
    """(count, mean, std) by the contract's tree, in float64."""
    n = adv.size
    pad = -(-n // ADV_CHUNK) * ADV_CHUNK
    m = np.zeros(pad)
    m[:n] = mask.ravel() != 0
    x = np.zeros(pad)
    x[:n] = adv.ravel().astype(np.float64)
    x = x * m
    total = np.zeros(3)
    for c in range(0, pad, ADV_CHUNK):
        s = np.stack([m[c:c + ADV_CHUNK], x[c:c + ADV_CHUNK], x[c:c + ADV_CHUNK] ** 2]).reshape(3, 256, 4)
        s = ((s[:, :, 0] + s[:, :, 1]) + s[:, :, 2]) + s[:, :, 3]
        while s.shape[1] > 1:
            w = s.shape[1] // 2
            s = s[:, :w] + s[:, w:]
        total = total + s[:, 0]
    if total[0] == 0:
        return 0.0, 0.0, 0.0
    mean = total[1] / total[0]
    return total[0], mean, np.sqrt(max(total[2] / total[0] - mean * mean, 0.0))


def adv_normalize(adv, mean, std):
    return ((adv.astype(np.float64) - mean) / (std + 1e-8)).astype(F32)


def loss(kind, p, action, logp, adv, ret, mask, scale_p, scale_v, clip_ratio, value_weight, entropy_weight, sigma=None):
    """A dict of float64: dp and mag [n, H + 1]; stat and stat_mag [n, 5] (policy loss, value loss, Hn, (r - 1) - d,
    r != rc); box: dsigma and dsigma_mag [n, H]; lp, d, active, near [n].  Everything from the float32 logits, value,
    sigma, lo, hi and ew, which take their float32 operations here too.  A masked row is zeros."""
    n, h = p.shape[0], p.shape[1] - 1
    live = mask != 0
    sp, sv, vw, nf = float(F32(scale_p)), float(F32(scale_v)), float(F32(value_weight)), float(F32(n))
    lo, hi = float(F32(1) - F32(clip_ratio)), float(F32(1) + F32(clip_ratio))
    ew = float(F32(entropy_weight) / F32(n))
    l = (p[:, :h].astype(F32) * F32(scale_p)).astype(np.float64)
    v = (p[:, h].astype(F32) * F32(scale_v)).astype(np.float64)
    adv, ret, logp = (x.astype(np.float64) for x in (adv, ret, logp))
    out = {}
    if kind == DISCRETE:
        x = l - l.max(axis=1, keepdims=True)
        e = np.exp(np.clip(x, -87.0, 0.0))
        s = e.sum(axis=1, keepdims=True)
        q, lq = e / s, x - np.log(s)
        hn = -(q * lq).sum(axis=1)
        lp = lq[np.arange(n), action]
        w = 1.0 + (np.abs(x) + np.abs(np.log(s))).max(axis=1) / 128.0
    else:
        sg = sigma.astype(np.float64)
        z, ls = (action.astype(np.float64) - l) / sg, np.log(sg)
        lp = (-0.5 * z * z - ls - C).sum(axis=1)
        hn = np.full(n, (K + ls).sum())
        w = 1.0 + (0.5 * z * z + np.abs(ls) + 0.92).sum(axis=1) / 2.0
    d = np.clip(lp - logp, -20.0, 20.0)
    r = np.exp(d)
    rc = np.clip(r, lo, hi)
    active = r * adv <= rc * adv
    g = np.where(active, -(adv * r) / nf, 0.0)
    dp, mag = np.zeros(p.shape), np.zeros(p.shape)
    if kind == DISCRETE:
        hit = np.arange(h)[None, :] == np.asarray(action)[:, None]
        dp[:, :h] = sp * (g[:, None] * (hit - q) + ew * q * (lq + hn[:, None]))
        mag[:, :h] = sp * w[:, None] * (np.abs(g)[:, None] * (hit + q) + ew * q * (np.abs(lq) + hn[:, None] + 1.0))
        hn_mag = w * (hn + 1.0)
    else:
        dp[:, :h] = sp * g[:, None] * z / sg
        mag[:, :h] = w[:, None] * np.abs(dp[:, :h])
        out["dsigma"] = np.where(live[:, None], g[:, None] * (z * z - 1.0) / sg - ew / sg, 0.0)
        out["dsigma_mag"] = np.where(live[:, None], w[:, None] * (np.abs(g)[:, None] * (z * z + 1.0) + ew) / sg, 0.0)
        hn_mag = np.full(n, (1.42 + np.abs(ls)).sum())
    dp[:, h] = 2.0 * vw * sv * (v - ret) / nf
    mag[:, h] = np.abs(dp[:, h])
    val = vw * (v - ret) ** 2
    stat = np.stack([-np.minimum(r * adv, rc * adv), val, hn, (r - 1.0) - d, (r != rc).astype(np.float64)], axis=1)
    stat_mag = np.stack([w * np.abs(adv) * np.maximum(r, rc), val, hn_mag, w * (r + 1.0), np.zeros(n)], axis=1)
    near = np.minimum(np.abs(r - lo), np.abs(r - hi)) <= 4 * 1.9e-5 * w * r
    z0 = np.where(live[:, None], 1.0, 0.0)
    out.update(dp=dp * z0, mag=mag * z0, stat=stat * z0, stat_mag=stat_mag * z0, lp=lp, d=d, active=active, near=near)
    return out


def stats_row(res, mask, rows):
    """The first five statistics and their bounds' magnitudes, the unmasked rows and the rows."""
    un = float((mask != 0).sum())
    div = un if un > 0 else 1.0
    return res["stat"].sum(axis=0) / div, res["stat_mag"].sum(axis=0) / div, un, float(rows)


def batch(kind, p, seed, scale_p, sigma=None, low=-1.0, high=1.0):
    """(action, logp, adv, ret, mask) for the head rows p: old log-probabilities that put d at -0.5, -0.1, 0.1, 0.5 in
    turn -- far from log(0.8) and log(1.2) --, advantages of both signs, row 1 masked, and for a Box head actions
    clamped to [low, high] with row 0 sitting on the upper bound."""
    rng = np.random.default_rng(seed)
    n, h = p.shape[0], p.shape[1] - 1
    if kind == DISCRETE:
        action = rng.integers(0, h, n).astype(np.int32)
    else:
        mu = (p[:, :h].astype(F32) * F32(scale_p))
        action = np.clip(mu + sigma * rng.standard_normal((n, h)).astype(F32), low, high).astype(F32)
        action[0, 0] = high
    adv = (rng.uniform(0.2, 2.0, n) * np.where(np.arange(n) % 3 == 0, -1.0, 1.0)).astype(F32)
    ret = rng.uniform(-1, 1, n).astype(F32)
    mask = np.ones(n, np.uint8)
    if n > 1:
        mask[1] = 0
    zero = np.zeros(n, F32)
    lp = loss(kind, p, action, zero, adv, ret, mask, scale_p, 1.0, 0.2, 0.5, 0.0, sigma)["lp"]
    d = np.array([-0.5, 0.5, -0.1, 0.1, 0.5, -0.5, 0.1, -0.1])[np.arange(n) % 8]
    return action, (lp - d).astype(F32), adv, ret, mask


def check_draw(kind, res, mask, action=None, low=-1.0, high=1.0):
    """The branches a loss case must reach, from the restatement alone."""
    live = mask != 0
    assert res["active"][live].any() and not res["active"][live].all()
    assert (res["d"][live] > 0).any() and (res["d"][live] < 0).any()
    assert not live.all() and not res["near"][live].any()
    assert kind == DISCRETE or ((action == high) | (action == low)).any()


def within(got, want, mag):
    """(ok, worst err / bound) of |got - want| <= kPpoErr * mag."""
    err, bound = np.abs(np.asarray(got, np.float64) - want), ERR * mag
    return bool(np.all(err <= bound)), float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
