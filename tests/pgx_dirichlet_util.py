"""The PUCT exploration contract (envpool_amd/csrc/pgx_dirichlet.hip.h) restated in numpy, independently of the header:
the draw indices, the boosted Marsaglia-Tsang gamma variates, the Dirichlet row in the lane group's summation order,
the mix, and the temperature weights with their pick.  Every float operation is one numpy float32 operation, so the
results are the header's bit for bit."""
import numpy as np

from actor_util import normal
from pgx_gumbel_util import exp_
from pgx_selfplay_util import SM, gumbel_log, key, puct_move, sample_at, uniform_of

F = np.float32
U64 = np.uint64
J = 16
BASE = 0x200
FLOOR = F(1e-30)
SCALE = F(1048576.0)


def index(a, j, c):
    return BASE + ((np.asarray(a, np.int64) * J + j) * 4 + c)


def draw(keys, idx):
    """U(idx) for keys [k] and indices [A] (or [k, A]): float32 [k, A]."""
    with np.errstate(over="ignore"):
        x = np.asarray(keys, dtype=U64)[:, None] + np.broadcast_to(np.asarray(idx, dtype=np.int64), (
            len(keys), np.shape(idx)[-1])).astype(U64)
    return uniform_of((SM(x) >> U64(41)).astype(np.uint32))


def params(alpha):
    """(alpha, d, c) as float32: d and c in float64 from the float32 alpha, rounded once."""
    alpha = F(alpha)
    d = (np.float64(alpha) + 1.0) - 1.0 / 3.0
    return alpha, F(d), F(1.0 / np.sqrt(9.0 * d))


def gamma(keys, actions, alpha):
    """(g float32 [k, A], fallback bool [k, A]) for the keys [k] and the actions 0 .. A-1."""
    alpha, d, c = params(alpha)
    acts = np.arange(actions)
    k = len(keys)
    y = np.full((k, actions), d, F)
    open_ = np.ones((k, actions), bool)
    for j in range(J):
        if not open_.any():
            break
        x = normal(draw(keys, index(acts, j, 0)))
        t = F(1.0) + c * x
        v = (t * t) * t
        ok = v > 0
        vs = np.where(ok, v, F(1.0)).astype(F)
        lhs = gumbel_log(draw(keys, index(acts, j, 1)))
        rhs = (((F(0.5) * x) * x + d) - d * vs) + d * gumbel_log(vs)
        acc = open_ & ok & (lhs < rhs)
        y = np.where(acc, d * vs, y).astype(F)
        open_ &= ~acc
    u2 = draw(keys, index(acts, J, 2))
    g = y * exp_(gumbel_log(u2) / alpha)
    g = np.where(g < FLOOR, FLOOR, g).astype(F)
    assert g.dtype == F
    return g, open_


def group(actions):
    lg = 1
    while lg < actions and lg < 64:
        lg <<= 1
    return lg, (actions + lg - 1) // lg


def row_sum(w):
    """S [k] of the terms w [k, A] (+0.0 where an action takes no part) in the contract's order."""
    k, actions = w.shape
    lg, e = group(actions)
    t = np.zeros((k, lg * e), F)
    t[:, :actions] = w
    t = t.reshape(k, lg, e)
    x = np.zeros((k, lg), F)
    for i in range(e):
        x = x + t[:, :, i]
    lanes = np.arange(lg)
    w_ = lg // 2
    while w_ >= 1:
        x = x + x[:, lanes ^ w_]
        w_ >>= 1
    assert x.dtype == F
    return x[:, 0]


def eta_rows(seed, env_ids, t, mask, alpha):
    """(eta float32 [k, A], fallbacks: the number of legal actions that took y = d)."""
    mask = np.asarray(mask) != 0
    g, fb = gamma(key(seed, env_ids, t), mask.shape[1], alpha)
    S = row_sum(np.where(mask, g, F(0.0)).astype(F))
    some = mask.any(axis=1)
    eta = np.where(mask, g / np.where(some, S, F(1.0)).astype(F)[:, None], F(0.0)).astype(F)
    return eta, int((fb & mask).sum())


def mix(prior, eta, mask, status, eps):
    """The mixed policy rows: legal entries of the rows with status 0."""
    eps = F(eps)
    om = F(1.0) - eps
    prior = np.asarray(prior, F)
    mixed = om * prior + eps * eta
    assert mixed.dtype == F
    take = (np.asarray(mask) != 0) & (np.asarray(status) == 0)[:, None]
    return np.where(take, mixed, prior).astype(F)


def weights(visits, T):
    """q uint32 [k, A]."""
    visits = np.asarray(visits, np.int64)
    vmax = np.maximum(visits.max(axis=1), 1)
    ratio = np.where(visits > 0, visits, vmax[:, None]).astype(F) / vmax.astype(F)[:, None]
    q = (exp_(gumbel_log(ratio) / F(T)) * SCALE).astype(np.uint32)
    return np.where(visits > 0, q, 0).astype(np.uint32)


def puct_move_temp(visits, result_action, elapsed, sample_plies, keys, T):
    """(action int32 [k], target float32 [k, A]) of the PUCT rule with a temperature."""
    action, target = puct_move(visits, result_action, elapsed, sample_plies, keys)
    if F(T) == F(1.0):
        return action, target
    visits = np.asarray(visits, np.int64)
    zero = (visits.sum(axis=1) == 0) | (np.asarray(result_action) < 0)
    q = weights(visits, T).astype(np.int64)
    r = sample_at(keys, q.sum(axis=1))
    sampled = (np.cumsum(q, axis=1) > r[:, None]).argmax(axis=1)
    take = ~zero & (np.asarray(elapsed) < sample_plies)
    return np.where(take, sampled, action).astype(np.int32), target
