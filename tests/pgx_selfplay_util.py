"""The self-play driver's contract (envpool_amd/csrc/pgx_selfplay.hip.h) restated in numpy: SM, the key, the uniform,
GumbelLog, noise rows, both move rules and the tally.  Every float operation is one numpy float32 operation, so the
results are the header's bit for bit."""
import numpy as np

F = np.float32
U64 = np.uint64
SAMPLE_SALT = 0x100
LN2_HI, LN2_LO = F(0.693359375), F(-2.12194440e-4)


def SM(x):
    """splitmix64 on uint64 arrays (mod 2^64)."""
    with np.errstate(over="ignore"):
        x = np.asarray(x, dtype=U64) + U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
        return x ^ (x >> U64(31))


def key(seed, env_ids, t):
    """key(e, t) for global env ids (array) and the ply counter t."""
    e = np.asarray(env_ids, dtype=np.int64).astype(np.uint32).astype(U64)
    return SM(U64(seed) ^ SM((e << U64(32)) | U64(int(t) & 0xFFFFFFFF)))


def uniform_of(n):
    """u of the 23-bit integer n."""
    return (np.asarray(n).astype(F) + F(0.5)) * F(2.0 ** -23)


def uniform(keys, actions):
    """u [len(keys), actions]."""
    with np.errstate(over="ignore"):
        x = np.asarray(keys, dtype=U64)[:, None] + np.arange(actions, dtype=U64)[None, :]
    return uniform_of((SM(x) >> U64(41)).astype(np.uint32))


def gumbel_log(x):
    x = np.asarray(x, dtype=F)
    m, e = np.frexp(x)
    m, e = m.astype(F), e.astype(np.int32)
    low = m < F(0.70710678)
    m = np.where(low, m * F(2.0), m).astype(F)
    e = np.where(low, e - 1, e)
    f = m - F(1.0)
    s = f / (F(2.0) + f)
    z = s * s
    p = np.full(x.shape, F(1.0) / F(9.0), dtype=F)
    p = p * z + F(1.0) / F(7.0)
    p = p * z + F(1.0) / F(5.0)
    p = p * z + F(1.0) / F(3.0)
    p = p * z
    s2 = F(2.0) * s
    r = s2 * p + s2
    fe = e.astype(F)
    out = fe * LN2_HI + (r + fe * LN2_LO)
    assert out.dtype == F
    return out


def noise_of(u):
    return -gumbel_log(-gumbel_log(u))


def noise_rows(seed, env_ids, t, actions, noise=True):
    """The [k, A] root noise of ply t for the listed global env ids."""
    if not noise:
        return np.zeros((len(env_ids), actions), F)
    return noise_of(uniform(key(seed, env_ids, t), actions))


def gumbel_move(action, weights):
    return np.where(action < 0, 0, action).astype(np.int32), np.asarray(weights, F)


def sample_at(keys, V):
    with np.errstate(over="ignore"):
        hi = SM(np.asarray(keys, dtype=U64) + U64(SAMPLE_SALT)) >> U64(32)
        return ((hi * np.asarray(V, dtype=U64)) >> U64(32)).astype(np.int64)


def puct_move(visits, result_action, elapsed, sample_plies, keys):
    """(action int32 [k], target float32 [k, A]) of the PUCT rule."""
    visits = np.asarray(visits, dtype=np.int64)
    k, a = visits.shape
    V = visits.sum(axis=1)
    zero = (V == 0) | (np.asarray(result_action) < 0)
    Vs = np.where(zero, 1, V)
    target = (visits.astype(F) / Vs.astype(F)[:, None]).astype(F)
    target[zero] = 0
    r = sample_at(keys, np.where(zero, 0, V))
    prefix = np.cumsum(visits, axis=1)
    sampled = (prefix > r[:, None]).argmax(axis=1)
    greedy = visits.argmax(axis=1)  # the first maximum: ties to the lowest action
    action = np.where(np.asarray(elapsed) < sample_plies, sampled, greedy)
    return np.where(zero, 0, action).astype(np.int32), target


def tally(done, reward, elapsed):
    """What a step's results add to (games, wins0, wins1, draws, plies)."""
    d = np.asarray(done).astype(bool).reshape(-1)
    r = np.asarray(reward, F).reshape(-1, 2)
    el = np.asarray(elapsed).reshape(-1)
    return np.array([d.sum(), (d & (r[:, 0] > 0)).sum(), (d & (r[:, 1] > 0)).sum(),
                     (d & (r[:, 0] == 0) & (r[:, 1] == 0)).sum(), el[d].sum()], dtype=np.int64)
