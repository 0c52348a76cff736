"""The rollout actor's contract (envpool_amd/csrc/actor.hip.h) restated in numpy, independently of the header: the
feature bytes, the key and the uniforms, ActorNormal, both heads and the blob written by hand.  Every float operation
is one numpy float32 (features: float64) operation, so the results are the header's bit for bit."""
import numpy as np

import pgx_net_util as nu
from pgx_gumbel_util import exp_
from pgx_selfplay_util import SM, gumbel_log, noise_of, uniform_of

F = np.float32
U64 = np.uint64
SALT = 0x41435452
MAGIC = 0x41415045
LOG_SQRT_2PI = F(0.9189385)


def features(obs, lo, scale):
    """uint8 [rows, F] of a list of observation arrays (one per obs key, in key order)."""
    x = np.concatenate([np.asarray(o).reshape(len(o), -1).astype(np.float64) for o in obs], axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        p = (x - np.asarray(lo, np.float64)) * np.asarray(scale, np.float64)
    fin = np.isfinite(p)
    return np.where(fin, np.clip(np.rint(np.where(fin, p, 0.0)), 0.0, 127.0), 0.0).astype(np.uint8)


def key(seed, env_ids, step):
    e = np.asarray(env_ids, dtype=np.int64).astype(np.uint32).astype(U64)
    with np.errstate(over="ignore"):
        return SM(U64(seed) ^ SM(SM(U64(int(step) & (2**64 - 1)) ^ U64(SALT)) + e))


def uniforms(keys, h):
    """u [len(keys), h]."""
    with np.errstate(over="ignore"):
        x = np.asarray(keys, dtype=U64)[:, None] + np.arange(h, dtype=U64)[None, :]
    return uniform_of((SM(x) >> U64(41)).astype(np.uint32))


def normal(u):
    """ActorNormal: PPND7 without its far tail, float32 throughout."""
    u = np.asarray(u, F)
    q = u - F(0.5)
    centre = np.abs(q) <= F(0.425)
    r = F(0.180625) - q * q
    num = ((F(5.9109374720e+01) * r + F(1.5929113202e+02)) * r + F(5.0434271938e+01)) * r + F(3.3871327179e+00)
    den = ((F(6.7187563600e+01) * r + F(7.8757757664e+01)) * r + F(1.7895169469e+01)) * r + F(1.0)
    inner = (q * num) / den
    t = np.where(q < 0, u, F(1.0) - u).astype(F)
    t = np.where(centre, F(0.25), t).astype(F)  # (any value inside the domain: the lane's result is not used)
    r = np.sqrt(-gumbel_log(t)).astype(F) - F(1.6)
    num = ((F(1.7023821103e-01) * r + F(1.3067284816e+00)) * r + F(2.7568153900e+00)) * r + F(1.4234372777e+00)
    den = (F(1.2021132975e-01) * r + F(7.3700164250e-01)) * r + F(1.0)
    v = num / den
    out = np.where(centre, inner, np.where(q < 0, -v, v))
    assert out.dtype == F
    return out


def discrete(p, scale_p, scale_v, seed, env_ids, step, deterministic):
    """(action int32 [rows], logp, value float32 [rows]) from the head's integers p [rows, H + 1]."""
    p = np.asarray(p, np.int32)
    h = p.shape[1] - 1
    logit = p[:, :h].astype(F) * F(scale_p)
    score = logit if deterministic else logit + noise_of(uniforms(key(seed, env_ids, step), h))
    action = score.argmax(axis=1).astype(np.int32)  # the first maximum: the lowest j
    top = logit.max(axis=1)
    total = np.zeros(len(p), F)
    for j in range(h):  # ascending j
        total = total + exp_(logit[:, j] - top)
    logp = (logit[np.arange(len(p)), action] - top) - gumbel_log(total)
    value = p[:, h].astype(F) * F(scale_v)
    assert logp.dtype == F and value.dtype == F
    return action, logp, value


def box(p, scale_p, scale_v, sigma, low, high, seed, env_ids, step, deterministic):
    """(action float32 [rows, H] -- clamped --, logp, value)."""
    p = np.asarray(p, np.int32)
    h = p.shape[1] - 1
    sigma, low, high = (np.asarray(x, F) for x in (sigma, low, high))
    mu = p[:, :h].astype(F) * F(scale_p)
    z = np.zeros_like(mu) if deterministic else normal(uniforms(key(seed, env_ids, step), h))
    raw = mu + sigma * z
    action = np.where(raw < low, low, np.where(raw > high, high, raw)).astype(F)
    terms = ((F(-0.5) * z) * z - gumbel_log(sigma)[None, :]) - LOG_SQRT_2PI
    logp = np.zeros(len(p), F)
    for j in range(h):
        logp = logp + terms[:, j]
    value = p[:, h].astype(F) * F(scale_v)
    assert logp.dtype == F and raw.dtype == F
    return action, logp, value


def make_blob(f, h, d, blocks, kind, layers, scale_p, scale_v, lo, scale, sigma=None, magic=MAGIC, version=1):
    """The blob by hand (no envpool_amd code)."""
    parts = [np.array([magic, version, f, h, d, blocks, kind], "<i4").tobytes(),
             np.array([scale_p, scale_v], "<f4").tobytes(), np.asarray(lo, "<f8").tobytes(),
             np.asarray(scale, "<f8").tobytes()]
    if kind == 1:
        parts.append(np.asarray(sigma, "<f4").tobytes())
    parts.append(nu.make_blob(f, h, d, blocks, layers, scale_p, scale_v)[32:].tobytes())
    return np.frombuffer(b"".join(parts), np.uint8).copy()


def head(layers, blocks, feat):
    """The head's integers int32 [rows, H + 1] of feature rows (pgx_net_util's int64 products)."""
    p, _ = nu.integers(layers, blocks, np.asarray(feat, np.uint8))
    return p.astype(np.int32)
