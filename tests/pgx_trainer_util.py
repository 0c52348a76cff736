"""Shared by the PGX trainer tests: numpy float64 restatements of the contract csrc/pgx_trainer.hip.h -- the loss, the
update rule with the norm's fixed-order sum, and the index hash -- and the minibatch every loss test uses."""
import numpy as np

LOSS_ERR = 2.0 ** -15  # kLossErr
CHUNK = 1024           # kTrainerChunk
M64 = (1 << 64) - 1


def mix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def index(seed, t, j, count):
    return (((mix(seed ^ mix((t << 32) | j)) >> 32) * count) >> 32) & 0xFFFFFFFF


def batch(rows, f, a, seed):
    """(obs, mask, pi, z): row 0 without a legal action, the last row with one, targets that do not sum to 1."""
    rng = np.random.default_rng(seed)
    obs = (rng.random((rows, f)) < 0.25).astype(np.uint8)
    mask = (rng.random((rows, a)) < 0.6).astype(np.uint8)
    mask[0] = 0
    mask[-1] = 0
    mask[-1, a // 2] = 1
    if rows == 1:
        mask[0, :2] = 1  # (one row: it has to carry a gradient)
    pi = (rng.random((rows, a)) * mask * 0.3).astype(np.float32)
    return obs, mask, pi, rng.uniform(-1, 1, rows).astype(np.float32)


def loss(p, mask, pi, z, scale_p, scale_v, value_weight):
    """(dp, its magnitudes, policy-loss sum / n, its magnitude, value-loss sum / n) in float64 from the float32 logits
    and value, which take one conversion and one multiply each."""
    n, a = mask.shape
    legal = mask != 0
    logit = (p[:, :a].astype(np.float32) * np.float32(scale_p)).astype(np.float64)
    v = (p[:, a].astype(np.float32) * np.float32(scale_v)).astype(np.float64)
    sp, sv, vw = float(np.float32(scale_p)), float(np.float32(scale_v)), float(np.float32(value_weight))
    m = np.where(legal, logit, -np.inf).max(axis=1, initial=-3.4e38)[:, None]
    e = np.where(legal, np.exp(np.clip(logit - m, -87.0, 0.0)), 0.0)
    S = e.sum(axis=1, keepdims=True)
    pi = np.where(legal, pi.astype(np.float64), 0.0)
    T = pi.sum(axis=1, keepdims=True)
    some = legal.any(axis=1, keepdims=True)
    q = np.where(some, e / np.where(some, S, 1.0), 0.0)
    dp = np.zeros(p.shape)
    dp[:, :a] = np.where(legal, sp * (T * q - pi) / n, 0.0)
    dp[:, a] = 2.0 * vw * sv * (v - z) / n
    mag = np.abs(dp)
    mag[:, :a] = np.where(legal, sp * (T * q + np.abs(pi)) / n, 0.0)
    log_s = np.log(np.where(some, S, 1.0))
    pol = np.where(some, T * (m + log_s), 0.0)[:, 0] - (pi * logit).sum(axis=1)
    pol_mag = np.where(some, T * (np.abs(m) + np.abs(log_s) + 1.0), 0.0)[:, 0] + np.abs(pi * logit).sum(axis=1)
    return dp, mag, pol.sum() / n, pol_mag.sum() / n, (vw * (v - z.astype(np.float64)) ** 2).sum() / n


def norm(grads):
    """The contract's fixed-order norm of the gradient arrays (weights, then biases)."""
    total = 0.0
    for g in grads:
        flat = np.zeros(-(-g.size // CHUNK) * CHUNK)
        flat[:g.size] = g.astype(np.float64).ravel()
        for chunk in flat.reshape(-1, 256, 4):
            sq = chunk * chunk
            s = ((sq[:, 0] + sq[:, 1]) + sq[:, 2]) + sq[:, 3]
            while len(s) > 1:
                s = s[:len(s) // 2] + s[len(s) // 2:]
            total = total + s[0]
    return np.sqrt(total)


class Rule:
    """The update of every array, float64, as the contract words it; `step(grads)` returns the norm."""

    def __init__(self, masters, optimizer, lr, momentum=0.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip=0.0):
        self.master = [np.array(m, np.float64) for m in masters]
        self.s1 = [np.zeros_like(m) for m in self.master]
        self.s2 = [np.zeros_like(m) for m in self.master]
        self.optimizer, self.lr, self.momentum, self.betas, self.eps = optimizer, lr, momentum, betas, eps
        self.weight_decay, self.clip, self.pow1, self.pow2 = weight_decay, clip, 1.0, 1.0

    def step(self, grads):
        n = norm(grads)
        scale = 1.0 if self.clip == 0.0 else min(1.0, self.clip / (n + 1e-6))
        self.pow1, self.pow2 = self.pow1 * self.betas[0], self.pow2 * self.betas[1]
        for i, grad in enumerate(grads):
            g = grad.astype(np.float64) * scale + self.weight_decay * self.master[i]
            if self.optimizer == "sgd":
                self.s1[i] = self.momentum * self.s1[i] + g
                self.master[i] = self.master[i] - self.lr * self.s1[i]
            else:
                lr_t = self.lr * np.sqrt(1.0 - self.pow2) / (1.0 - self.pow1)
                self.s1[i] = self.betas[0] * self.s1[i] + (1.0 - self.betas[0]) * g
                self.s2[i] = self.betas[1] * self.s2[i] + ((1.0 - self.betas[1]) * g) * g
                self.master[i] = self.master[i] - (lr_t * self.s1[i]) / (np.sqrt(self.s2[i]) + self.eps)
        return n

    def quantised(self, i, weight):
        top = 127 if weight else 1 << 30
        return np.clip(np.rint(self.master[i]), -top, top).astype(np.int8 if weight else np.int32)
