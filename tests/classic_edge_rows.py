"""One-step boundary lattices for classic_control (test infrastructure).

`lattice(task, version)` builds a few thousand crafted fp64 states with crafted actions, to be `set_state`-ed into a
pool and stepped ONCE.  Rows sit on the thresholds that decide `done`, a clamp or a wrap, on either side of them:

* trig-free rows: the deciding quantity has no sin / cos in it, so the threshold itself, the next double above and
  the next below are constructible (CartPole's x and theta with zero velocity);
* margin rows: the deciding quantity passes through libm, so the state is placed where the quantity lands at
  threshold +- DELTA and well beyond.  DELTA = 1e-9 is about 10^7 times the 1-ulp fp64 difference that device
  sin / cos may have, and about 100 times below what a float32 near 1 resolves: a decision taken on float32 values,
  or with `>=` for `>`, flips, a correct kernel cannot;
* action rows: integers outside the action range (their meaning is the reference's `else` branch, or its `act - 1`
  arithmetic) and float actions at, next to and far beyond the clip, signed zeros, infinities and NaN.
  Left out on purpose: INT_MIN for MountainCar and Acrobot (`act - 1` overflows in the reference itself:
  undefined), and INT_MIN / INT_MAX for Acrobot (a torque of 2e9 sends the angles to 1e7 rad, and the reference's
  `while (theta >= pi)` wraps then spin for millions of trips on either side).

Every group of rows carries `expect(post_state, frame) -> bool rows`: which side of the decision the port must have
taken, checked on the CPU (tests/test_oracle_scripted.py) before any kernel sees the rows.  All states are finite,
angles inside (-2 pi, 2 pi), velocities inside twice their clamps.
"""
import numpy as np

DELTA = 1e-9
LIMIT = 200            # max_episode_steps of the lattice pools
N_ROWS = 3001          # not a multiple of 64: the last wave is ragged
I32 = np.iinfo(np.int32)
PI = np.pi
NS = {"CartPole": 4, "Pendulum": 2, "MountainCar": 2, "MountainCarContinuous": 2, "Acrobot": 5}


def f32_neighbours(v):
    v = np.float32(v)
    return [v, np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))]


def float_actions(limit):
    out = []
    for s in (1.0, -1.0):
        out += f32_neighbours(s * limit) + [np.float32(s * 2.5), np.float32(s * 0.0), np.float32(s * np.inf)]
    return np.array(out + [np.float32(np.nan)], dtype=np.float32)


class Rows:
    def __init__(self, ns, float_action):
        self.ns, self.float_action = ns, float_action
        self.state, self.action, self.cur, self.done, self.groups = [], [], [], [], []
        self.n = 0

    def add(self, name, state, action, expect=None, cur=None):
        state = np.atleast_2d(np.asarray(state, dtype=np.float64))
        k = state.shape[0]
        action = np.broadcast_to(np.asarray(action, dtype=np.float32 if self.float_action else np.int32), (k,))
        cur = np.where(np.arange(k) % 5 == 4, LIMIT - 1, 5) if cur is None else np.broadcast_to(cur, (k,))
        self.state.append(state)
        self.action.append(action)
        self.cur.append(np.asarray(cur, dtype=np.int64))
        self.done.append(np.zeros(k, dtype=bool))
        if expect is not None:
            self.groups.append((name, slice(self.n, self.n + k), expect))
        self.n += k

    def finish(self, bulk):
        """Fill up to N_ROWS with `bulk(k)` = random (state, action) rows, every 97th of them a done env (it resets
        in the same launch)."""
        k = N_ROWS - self.n
        assert k > 64, self.n
        state, action = bulk(k)
        self.add("bulk", state, action)
        self.done[-1][::97] = True
        out = dict(state=np.concatenate(self.state), action=np.concatenate(self.action),
                   cur=np.concatenate(self.cur), done=np.concatenate(self.done), groups=self.groups)
        assert out["state"].shape == (N_ROWS, self.ns) and np.isfinite(out["state"]).all()
        return out


def product(*lists):
    grids = np.meshgrid(*[np.arange(len(v)) for v in lists], indexing="ij")
    return [np.asarray(v)[g.reshape(-1)] for v, g in zip(lists, grids)]


def near(a, b):
    return np.abs(a - b) <= 1e-12


# ---------------------------------------------------------------------------------------------------------------
def cartpole(rng):
    r = Rows(4, False)
    thr_x, thr_t = 2.4, 12 * 2 * PI / 360
    acts = [0, 1, -1, 2, 7, I32.min, I32.max]

    def expect(state, cur):
        # trig-free: x' = x + tau * x_dot and theta' = theta + tau * theta_dot are the port's own values
        x = state[:, 0] + 0.02 * state[:, 1]
        t = state[:, 2] + 0.02 * state[:, 3]
        over = (x < -thr_x) | (x > thr_x) | (t < -thr_t) | (t > thr_t)
        lim = cur + 1 >= LIMIT
        return lambda post, f: (f["done"][:, 0] == (over | lim)) & (f["trunc"][:, 0] == lim)

    def add(name, state, action, cur):
        r.add(name, state, action, expect(np.asarray(state), np.asarray(cur)), cur)

    for col, thr in ((0, thr_x), (2, thr_t)):
        vals = [s * v for s in (1, -1) for v in (thr, np.nextafter(thr, np.inf), np.nextafter(thr, 0))]
        v, a, c = product(vals, acts, [5, LIMIT - 1])
        state = np.zeros((len(v), 4))
        state[:, col] = v
        add(f"exact threshold, column {col}", state, a, c)
        # with a velocity: the state placed so that the stepped value lands at the threshold +- DELTA and beyond
        k = 256
        vel = rng.uniform(-2, 2, k)
        m = np.resize([DELTA, -DELTA, 0.3 * thr, -0.3 * thr], k)
        sign = np.resize([1, 1, 1, 1, -1, -1, -1, -1], k)
        state = np.zeros((k, 4))
        state[:, col] = sign * (thr + m) - 0.02 * vel
        state[:, col + 1] = vel
        if col == 0:  # a pole that is not upright, inside its threshold
            state[:, 2] = rng.uniform(-0.1, 0.1, k)
        add(f"margin, column {col}", state, rng.integers(0, 2, k), np.where(np.arange(k) % 7 == 6, LIMIT - 1, 5))

    def bulk(k):
        return rng.uniform(-1, 1, (k, 4)) * [2.6, 2.0, 0.25, 2.5], rng.integers(-1, 3, k)
    return r.finish(bulk)


# ---------------------------------------------------------------------------------------------------------------
def mountain_car(rng, continuous):
    r = Rows(2, continuous)
    gain, goal = (0.0015, 0.45) if continuous else (0.001, 0.5)
    lo, hi, vmax, grav = -1.2, 0.6, 0.07, 0.0025

    def actions(k):
        return rng.uniform(-1.3, 1.3, k).astype(np.float32) if continuous else rng.integers(0, 3, k)

    def inc(a, pos):  # what the step adds to vel, in the port's operation order
        a = np.clip(np.asarray(a, dtype=np.float64), -1, 1) if continuous else np.asarray(a, dtype=np.float64) - 1
        return a * gain - np.cos(3 * pos) * grav

    def margins(k, big):
        return np.resize([DELTA, -DELTA, big, -big], k)

    k = 128
    cur5 = np.full(k, 5)
    for s in (1, -1):  # the speed clamp on either side
        m, a, pos = margins(k, 0.03), actions(k), rng.uniform(-1.0, 0.3, k)
        pre = s * (vmax + m)
        r.add(f"speed clamp {s * vmax}", np.stack([pos, pre - inc(a, pos)], 1), a,
              lambda post, f, m=m, pre=pre, s=s: np.where(m > 0, post[:, 1] == s * vmax,
                                                           near(post[:, 1], pre) & (np.abs(post[:, 1]) < vmax)), cur5)
    # the wall: pos' = -1.2 +- margin with vel' < 0; clamped rows have vel zeroed
    m, a, v = margins(k, 0.005), actions(k), rng.uniform(-0.06, -0.01, k)
    pos = (lo + m) - v
    r.add("wall", np.stack([pos, v - inc(a, pos)], 1), a,
          lambda post, f, m=m, v=v: np.where(m < 0, (post[:, 0] == lo) & (post[:, 1] == 0),
                                             (post[:, 0] > lo) & near(post[:, 1], v)), cur5)
    # a car set beyond the wall that moves right: clamped to the wall, vel kept
    a, v = actions(32), rng.uniform(0.005, 0.03, 32)
    pos = np.full(32, -1.25)
    r.add("wall, moving right", np.stack([pos, v - inc(a, pos)], 1), a,
          lambda post, f, v=v: (post[:, 0] == lo) & near(post[:, 1], v) & ~f["done"][:, 0], np.full(32, 5))
    # the clamp at 0.6 (beyond the goal: done either way)
    m, a, v = margins(k, 0.005), actions(k), rng.uniform(0.01, 0.06, k)
    pos = (hi + m) - v
    r.add("position clamp 0.6", np.stack([pos, v - inc(a, pos)], 1), a,
          lambda post, f, m=m: np.where(m > 0, post[:, 0] == hi, post[:, 0] < hi) & f["done"][:, 0] & ~f["trunc"][:, 0],
          cur5)
    # the goal: position at goal +- margin with vel' > 0, and vel' = +- margin beyond the goal position
    m, a, v = margins(k, 0.05), actions(k), rng.uniform(0.005, 0.06, k)
    pos = (goal + m) - v
    r.add("goal position", np.stack([pos, v - inc(a, pos)], 1), a,
          lambda post, f, m=m: f["done"][:, 0] == (m > 0), cur5)
    m, a = margins(k, 0.01), actions(k)
    pos = (goal + 0.03) - m
    r.add("goal velocity", np.stack([pos, m - inc(a, pos)], 1), a,
          lambda post, f, m=m: f["done"][:, 0] == (m > 0), cur5)
    if continuous:
        r.add("goal reward", np.stack([np.full(8, 0.47), np.full(8, 0.02)], 1), np.float32(0.5),
              lambda post, f: f["reward"][:, 0] == np.float32(-0.1 * 0.5 * 0.5 + 100), np.full(8, 5))
    # the step limit together with the goal
    a = actions(16)
    r.add("goal at the step limit", np.stack([np.full(16, goal + 0.01), np.full(16, 0.02)], 1), a,
          lambda post, f: f["done"][:, 0] & f["trunc"][:, 0], np.full(16, LIMIT - 1))
    # actions
    special = float_actions(1.0) if continuous else np.array([-1, 3, 8, I32.max], dtype=np.int32)
    pos, a = product([-0.9, -0.5, 0.3, 0.46], special)
    r.add("actions", np.stack([pos, np.full(len(pos), 0.01)], 1), a)

    def bulk(k):
        return rng.uniform(-1, 1, (k, 2)) * [0.9, 0.07] - [0.3, 0.0], actions(k)
    return r.finish(bulk)


# ---------------------------------------------------------------------------------------------------------------
def pendulum(rng, version):
    r = Rows(2, True)
    k = 256
    cur5 = np.full(k, 5)

    def torque(theta, act):  # 3 * (g / 2 * sin(theta) + u) * dt in the port's operation order
        u = np.clip(np.asarray(act, dtype=np.float64), -2, 2)
        return 3 * (10.0 / 2 * np.sin(theta) + u) * 0.05

    for s in (1, -1):  # the speed clamp
        m = np.resize([DELTA, -DELTA, 3.0, -3.0], k)
        theta, act = rng.uniform(-3, 3, k), rng.uniform(-2.5, 2.5, k).astype(np.float32)
        pre = s * (8 + m)
        r.add(f"speed clamp {8 * s}", np.stack([theta, pre - torque(theta, act)], 1), act,
              lambda post, f, m=m, pre=pre, s=s: np.where(m > 0, post[:, 1] == 8 * s,
                                                           near(post[:, 1], pre) & (np.abs(post[:, 1]) < 8)), cur5)
    for s in (1, -1):  # the wrap: theta' = +-pi +- margin.  theta starts 1e-4 .. 1e-3 short of +-pi, where
        # sin(theta) is so small that a last-bit difference of it cannot reach theta'
        m = np.resize([DELTA, -DELTA, 0.2, -0.2], k)
        theta = s * (PI - rng.uniform(1e-4, 1e-3, k))
        act = rng.uniform(-2.5, 2.5, k).astype(np.float32)
        speed = ((s * PI + m) - theta) / 0.05
        state = np.stack([theta, speed - torque(theta, act)], 1)
        pre = theta + (state[:, 1] + torque(theta, act)) * 0.05  # the port's theta before its wrap
        assert (np.abs(np.abs(pre - s * PI) - np.abs(m)) < 1e-14).all()
        want = np.where(pre >= PI, pre - 2 * PI, np.where(pre < -PI, pre + 2 * PI, pre))
        r.add(f"wrap at {s} pi", state, act, lambda post, f, want=want: near(post[:, 0], want), cur5)
    r.add("step limit", np.stack([np.full(8, 0.5), np.full(8, 1.0)], 1), np.float32(0.5),
          lambda post, f: f["done"][:, 0] & f["trunc"][:, 0], np.full(8, LIMIT - 1))
    theta, a = product([0.5, -2.0, 3.0], float_actions(2.0))
    r.add("actions", np.stack([theta, np.full(len(theta), 1.0)], 1), a)

    def bulk(k):
        return rng.uniform(-1, 1, (k, 2)) * [PI, 8], rng.uniform(-2.5, 2.5, k).astype(np.float32)
    return r.finish(bulk)


# ---------------------------------------------------------------------------------------------------------------
def acrobot_derivs(s):
    g, l, m, lc, i = 9.8, 1.0, 1.0, 0.5, 1.0
    t1, t2, d1_, d2_, a = s
    d1 = m * lc * lc + m * (l * l + lc * lc + 2 * l * lc * np.cos(t2)) + i * 2
    d2 = m * (lc * lc + l * lc * np.cos(t2)) + i
    phi2 = m * lc * g * np.cos(t1 + t2 - PI / 2)
    phi1 = -(d2_ + 2 * d1_) * m * l * lc * d2_ * np.sin(t2) + m * (lc + l) * g * np.cos(t1 - PI / 2) + phi2
    dd2 = (a + d2 / d1 * phi1 - m * l * lc * d1_ * d1_ * np.sin(t2) - phi2) / (m * lc * lc + i - d2 * d2 / d1)
    dd1 = -(d2 * dd2 + phi1) / d1
    return np.stack([d1_, d2_, dd1, dd2, np.zeros_like(a)])


def acrobot_rk4(state, torque):
    """The textbook Acrobot's RK4 step of 0.2 s: [k, 4] states before the wraps and the clamps."""
    y0 = np.concatenate([state[:, :4].T, torque[None, :]])
    dt = 0.2
    k1 = acrobot_derivs(y0)
    k2 = acrobot_derivs(y0 + k1 * (dt / 2))
    k3 = acrobot_derivs(y0 + k2 * (dt / 2))
    k4 = acrobot_derivs(y0 + k3 * dt)
    return (y0 + (k1 + k2 * 2 + k3 * 2 + k4) * (dt / 6.0))[:4].T


ACROBOT_DECISIONS = ("height", "d1 clamp +", "d1 clamp -", "d2 clamp +", "d2 clamp -",
                     "wrap1 +", "wrap1 -", "wrap2 +", "wrap2 -")


ACROBOT_PLACED = ACROBOT_DECISIONS[:5]


def acrobot_sides(pre):
    """Per decision: (margin to its threshold, side taken) of rows `pre` = the state after RK4."""
    def wrapped(x):
        return x - 2 * PI * np.floor((x + PI) / (2 * PI))
    t1, t2 = wrapped(pre[:, 0]), wrapped(pre[:, 1])
    h = -np.cos(t1) - np.cos(t1 + t2) - 1
    out = {"height": (np.abs(h), h > 0)}
    for name, v, lim in (("d1", pre[:, 2], 4 * PI), ("d2", pre[:, 3], 9 * PI)):
        out[name + " clamp +"] = (np.abs(v - lim), v > lim)
        out[name + " clamp -"] = (np.abs(v + lim), v < -lim)
    for name, v in (("wrap1", pre[:, 0]), ("wrap2", pre[:, 1])):
        # the wraps decide at every odd multiple of pi on the way: the distance to the nearest one
        dist = np.abs(wrapped(v - PI))
        out[name + " +"] = (dist, v >= PI)
        out[name + " -"] = (dist, v < -PI)
    return out


def acrobot_decision_values(pre):
    """Per decision, the deciding quantity minus its threshold (its sign is the side) of rows `pre`."""
    return {
        "height": -np.cos(pre[:, 0]) - np.cos(pre[:, 0] + pre[:, 1]) - 1,
        "d1 clamp +": pre[:, 2] - 4 * PI, "d1 clamp -": pre[:, 2] + 4 * PI,
        "d2 clamp +": pre[:, 3] - 9 * PI, "d2 clamp -": pre[:, 3] + 9 * PI,
        "wrap1 +": pre[:, 0] - PI, "wrap1 -": pre[:, 0] + PI, "wrap2 +": pre[:, 1] - PI, "wrap2 -": pre[:, 1] + PI,
    }


def acrobot_placed(state, torque, decision, pairs=48):
    """Rows whose deciding quantity lands 2 DELTA (within DELTA / 2) on either side of the threshold: RK4 has no
    closed form to invert, so the row is searched by bisection along the segment between two sampled states that
    lie on different sides (a segment stays inside the sampled box)."""
    def value(s, tq):
        return acrobot_decision_values(acrobot_rk4(s, tq))[decision]
    below = np.nonzero(value(state, torque) < -1e-3)[0][:pairs]
    out_s, out_t = [], []
    for target in (2 * DELTA, -2 * DELTA):
        a = state[below]
        tq = torque[below]
        # partners: for every `a`, some sampled state that is above the threshold under a's own torque
        b = np.empty_like(a)
        found = np.zeros(len(a), dtype=bool)
        for shift in range(1, 400):
            cand = state[(below + shift * 7) % len(state)]
            ok = ~found & (value(cand, tq) > 1e-3)
            b[ok] = cand[ok]
            found |= ok
            if found.all():
                break
        a, b, tq = a[found], b[found], tq[found]
        lo, hi = np.zeros(len(a)), np.ones(len(a))
        for _ in range(70):
            mid = 0.5 * (lo + hi)
            up = value(a + mid[:, None] * (b - a), tq) > target
            hi = np.where(up, mid, hi)
            lo = np.where(up, lo, mid)
        rows = a + hi[:, None] * (b - a)
        good = np.abs(value(rows, tq) - target) <= DELTA / 2
        out_s.append(rows[good])
        out_t.append(tq[good])
    return np.concatenate(out_s), np.concatenate(out_t)


def acrobot(rng):
    r = Rows(5, False)
    k = 1800
    state = np.zeros((k, 5))
    state[:, 0:2] = rng.uniform(-PI, PI, (k, 2))
    state[:, 2] = rng.uniform(-8 * PI, 8 * PI, k) * rng.uniform(0, 1, k)
    state[:, 3] = rng.uniform(-18 * PI, 18 * PI, k) * rng.uniform(0, 1, k)
    state[:, 4] = rng.integers(-1, 2, k)  # the torque of the step before: overwritten
    act = rng.integers(0, 3, k)
    act[::50] = np.resize([-1, 3, 8], len(act[::50]))
    # dense rows, then per decision the rows placed 2 DELTA on either side of its threshold.  Not for the wraps: 2e-9
    # from +-pi the observation sin(theta) is 2e-9 itself, and the 1e-15 that last-bit differences of libm leave in
    # theta is 5e-7 of it, more than the 4 ulp(fp32) the observations are held to; the wraps keep their dense rows
    placed = [acrobot_placed(state, act.astype(np.float64) - 1, d) for d in ACROBOT_PLACED]
    n_placed = sum(len(p[0]) for p in placed)
    state = np.concatenate([state] + [p[0] for p in placed])
    act = np.concatenate([act] + [np.rint(p[1]).astype(np.int64) + 1 for p in placed])
    pre = acrobot_rk4(state, act.astype(np.float64) - 1)
    sides = acrobot_sides(pre)
    margin = np.min([sides[d][0] for d in ACROBOT_DECISIONS], axis=0)
    keep = margin >= DELTA
    stats = {"dropped": float(1 - keep.mean()), "placed": n_placed}
    for d in ACROBOT_DECISIONS:
        close = keep & (sides[d][0] <= 3 * DELTA)
        stats[d] = (int((sides[d][1] & keep).sum()), int((~sides[d][1] & keep).sum()),
                    int((sides[d][1] & close).sum()), int((~sides[d][1] & close).sum()))
    state, act, pre = state[keep], act[keep], pre[keep]
    sides = acrobot_sides(pre)

    def expect(post, f):
        want = pre.copy()
        want[:, 0:2] -= 2 * PI * np.floor((want[:, 0:2] + PI) / (2 * PI))
        want[:, 2] = np.clip(want[:, 2], -4 * PI, 4 * PI)
        want[:, 3] = np.clip(want[:, 3], -9 * PI, 9 * PI)
        up = sides["height"][1]
        lim = f["elapsed_step"][:, 0] >= LIMIT
        return ((np.abs(post[:, :4] - want) <= 1e-10).all(axis=1) & (f["done"][:, 0] == (up | lim)) &
                (f["reward"][:, 0] == np.where(up, 0, -1)) & (f["trunc"][:, 0] == lim))
    r.add("dense and placed", state, act, expect)

    def bulk(k):
        s = rng.uniform(-1, 1, (k, 5)) * [PI, PI, 4 * PI, 9 * PI, 1]
        return s, rng.integers(0, 3, k)
    out = r.finish(bulk)
    out["stats"] = stats
    return out


LATTICES = {
    "CartPole": ("CartPole", 0), "Pendulum-v0": ("Pendulum", 0), "Pendulum-v1": ("Pendulum", 1),
    "MountainCar": ("MountainCar", 0), "MountainCarContinuous": ("MountainCarContinuous", 0),
    "Acrobot": ("Acrobot", 0),
}
_cache = {}


def lattice(name):
    """(task, version, rows) of a lattice; built once and shared (read only)."""
    if name not in _cache:
        task, version = LATTICES[name]
        rng = np.random.default_rng(2024)
        rows = {"CartPole": cartpole, "Pendulum": lambda g: pendulum(g, version),
                "MountainCar": lambda g: mountain_car(g, False),
                "MountainCarContinuous": lambda g: mountain_car(g, True), "Acrobot": acrobot}[task](rng)
        for v in rows.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = (task, version, rows)
    return _cache[name]


def flat_state(rows, width):
    """[s..., done, cur_step] rows, the s part padded with zeros to `width` columns (the port's hook takes 5)."""
    s = rows["state"]
    pad = np.zeros((s.shape[0], width - s.shape[1]))
    return np.concatenate([s, pad, rows["done"][:, None].astype(np.float64), rows["cur"][:, None].astype(np.float64)],
                          axis=1)
