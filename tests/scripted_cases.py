"""Scripted closed-loop cases for classic_control and toy_text (test infrastructure).

Uniformly random play from a reset state never takes most of the branches that decide `done` and the large rewards
of these envs (the goal and the wall of the MountainCars, CartPole's x threshold, Acrobot's termination, the goal
cell of CliffWalking, Taxi's pickup / drop-off cases ...).  Every case below is a POLICY that looks at the
observations it is handed and steers an 8-env pool into those branches, plus the EVENTS the case exists for, as
predicates on the recorded rollout.  tests/golden/make_scripted_golden.py runs the policies against the reference
compiled in place and writes tests/golden/scripted_<case>.npz (asserting the events first);
tests/test_oracle_scripted.py and tests/test_gpu_classic_toy_edges.py replay those files open loop through the port
and the kernels, and check that the committed files still hold their events.

case table (events = what the fixture is asserted to contain; "set_state only" = no reference trajectory takes the
branch, it is pinned against the port alone by the one-step lattices of tests/classic_edge_rows.py):

  mountaincar_pump      goal termination (done, not trunc, pos >= 0.5), the wall (pos == -1.2 with vel == 0)
  mountaincar_wall      no step limit; the car is pushed back down the right hill short of the goal and action 0 is
                        held for stretches: the wall again and again, and the speed clamp at -0.07 on the way there
                        set_state only: the speed clamp at +0.07 (no policy tried here reached it), the position
                        clamp at 0.6 (the episode ends at 0.5, and one step from below 0.5 adds less than 0.07)
  mountaincarcont_pump  actions +-1.5 (the clip), the wall, the goal with reward 100 - 0.1 * 1.5^2 = 99.775
  cartpole_drift        a balancing controller with a bias per env: termination on x < -2.4 and on x > 2.4 with the
                        pole upright (every termination of random play is theta)
  acrobot_pump          no step limit; terminations with reward 0, d(theta1) saturated at 4 pi (one sign)
                        set_state only: the other sign of that clamp, and the 9 pi clamp of d(theta2) (no policy
                        tried here got past 23.5 of 28.3: pumping on either joint velocity, on their sum or
                        difference, bang-bang on the sign of theta2, constant torque)
  pendulum_v0_spin      torque held at +-2.5 (both signs of the clip) until the speed sits at +-8 (both clamps)
  pendulum_v1_spin      the same under version 1's update order
  cliffwalking_paths    the safe path to the goal cell 47 (done), walks into the cliff at every column (-100)
  cliffwalking_slippery closed loop along the top rows until the goal is reached
  taxi_script           decode obs, pick up, drop off (20, done); a pickup away from the passenger (-10), a pickup
                        while carrying at all 25 cells (-10), a drop-off with an empty taxi (-10), a drop-off at
                        another depot while carrying (set down there, -1), a move into every wall segment and border
  nchain_hold           action 0 held: the 10 reward at the end of the chain and the slip (reward 2 under action 0)
  frozenlake_goal       value-iteration policy under the true slip: goal (reward 1) and hole terminations
  frozenlake8x8_goal    the same on the 8x8 map
"""
import numpy as np

N = 8          # envs per fixture
SEED = 3       # seed of the committed fixtures
LIVE_SEED = 11  # seed of the live port-vs-reference run (tests/test_oracle_scripted.py)

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------
# policies: make(n) -> policy(t, frame) -> actions; `frame` is the dict the pool returned last (rows [n, elems])
# ---------------------------------------------------------------------------------------------------------------
def mountaincar_pump(n):
    return lambda t, f: np.where(f["obs"][:, 1] >= 0, 2, 0).astype(np.int32)


def mountaincar_wall(n):
    def policy(t, f):
        a = np.where(f["obs"][:, 1] >= 0, 2, 0)
        a = np.where(f["obs"][:, 0] > 0.2, 0, a)  # pushed back down the right hill, short of the goal
        if (t % 100) >= 60:  # a stretch of constant action 0 after 60 steps of pumping
            a[:] = 0
        return a.astype(np.int32)
    return policy


def mountaincarcont_pump(n):
    return lambda t, f: np.where(f["obs"][:, 1] >= 0, 1.5, -1.5).astype(F32).reshape(-1, 1)


CARTPOLE_BIAS = np.array([0.1, 0.1, 0.1, 0.1, -0.1, -0.1, -0.1, -0.1])


def cartpole_drift(n):
    bias = np.resize(CARTPOLE_BIAS, n)
    return lambda t, f: (3.0 * f["obs"][:, 2] + f["obs"][:, 3] + bias > 0).astype(np.int32)


def acrobot_pump(n):
    return lambda t, f: np.where(f["obs"][:, 5] >= 0, 2, 0).astype(np.int32)


def pendulum_spin(n):
    def policy(t, f):
        # +2.5 for an episode of 200 steps, -2.5 for the next (odd envs the other way round); every 25th step a
        # torque inside the limits, so the unclipped branch is in the file as well
        sign = np.where((np.arange(n) + t // 200) % 2 == 0, 1.0, -1.0)
        a = 2.5 * sign
        if t % 25 == 24:
            a = 0.75 * sign
        return a.astype(F32).reshape(-1, 1)
    return policy


def cliffwalking_paths(n):
    def policy(t, f):
        obs = f["obs"][:, 0]
        x, y = obs // 12, obs % 12
        a = np.zeros(n, dtype=np.int32)
        for e in range(n):
            # even envs take the safe path (up, along row 2, down at the last column); odd envs step down into the
            # cliff at a column of their own that moves on with every attempt
            col = 11 if e % 2 == 0 else 1 + (e // 2 + 4 * (t // 28)) % 10
            if x[e] == 3 and y[e] == 0:
                a[e] = 0
            elif y[e] < col:
                a[e] = 1
            else:
                a[e] = 2
        return a
    return policy


def cliffwalking_slippery(n):
    def policy(t, f):
        obs = f["obs"][:, 0]
        x, y = obs // 12, obs % 12
        # keep to the two top rows (a slip is perpendicular to the move); go down only in the last column
        return np.where(y == 11, 2, np.where(x >= 2, 0, 1)).astype(np.int32)
    return policy


# Taxi: the map of gym's Taxi-v3 (rows x, columns y).  East of (x, y) is open iff MAP[x][y + 1] == ':', west iff
# MAP[x][y] == ':'; actions 0 south (x + 1), 1 north, 2 east (y + 1), 3 west, 4 pickup, 5 drop-off.
TAXI_MAP = ("|:|::|", "|:|::|", "|::::|", "||:|:|", "||:|:|")
TAXI_LOC = ((0, 0), (0, 4), (4, 0), (4, 3))


def taxi_open(x, y, a):
    if a == 0:
        return x < 4
    if a == 1:
        return x > 0
    if a == 2:
        return TAXI_MAP[x][y + 1] == ":"
    return TAXI_MAP[x][y] == ":"


TAXI_BLOCKED = [(x, y, a) for x in range(5) for y in range(5) for a in range(4) if not taxi_open(x, y, a)]
_DX, _DY = (1, -1, 0, 0), (0, 0, 1, -1)


def taxi_toward(x, y, tx, ty):
    """First move of a shortest path (x, y) -> (tx, ty); None when already there."""
    if (x, y) == (tx, ty):
        return None
    dist = {(tx, ty): 0}
    todo = [(tx, ty)]
    while todo:
        cx, cy = todo.pop(0)
        for a in range(4):
            px, py = cx - _DX[a], cy - _DY[a]  # (px, py) --a--> (cx, cy)
            if 0 <= px < 5 and 0 <= py < 5 and taxi_open(px, py, a) and (px, py) not in dist:
                dist[(px, py)] = dist[(cx, cy)] + 1
                todo.append((px, py))
    for a in range(4):
        if taxi_open(x, y, a) and dist.get((x + _DX[a], y + _DY[a]), 99) == dist[(x, y)] - 1:
            return a
    raise AssertionError("taxi map is connected")


def taxi_decode(obs):
    return obs // 100, (obs // 20) % 5, (obs // 4) % 5, obs % 4


def taxi_programs(n):
    """Per env, the list of tasks of its first episode; afterwards every episode is a plain delivery.
    ("at", x, y, a): drive to the cell and do `a` there; ("fetch",): drive to the passenger and pick up;
    ("deliver",): drive to the destination and drop off; ("wrong",): drive to a depot that is not the
    destination, drop off and pick up again."""
    progs = []
    share = -(-len(TAXI_BLOCKED) // max(1, n - 1))
    for e in range(n):
        if e == n - 1:  # the last env: every failing pickup and drop-off case
            p = [("at", 2, 2, 4), ("at", 2, 2, 5), ("fetch",)]
            p += [("at", x, y if x % 2 == 0 else 4 - y, 4) for x in range(5) for y in range(5)]
            p += [("at", 2, 2, 5), ("wrong",), ("deliver",)]
        else:  # a share of the blocked moves, empty and carrying
            mine = TAXI_BLOCKED[e * share:(e + 1) * share]
            half = len(mine) // 2
            p = [("at", x, y, a) for x, y, a in mine[:half]] + [("fetch",)]
            p += [("at", x, y, a) for x, y, a in mine[half:]] + [("wrong",), ("deliver",)]
        progs.append(p)
    return progs


def taxi_script(n):
    progs = taxi_programs(n)
    sub = [0] * n  # progress inside ("wrong",)

    def policy(t, f):
        a = np.zeros(n, dtype=np.int32)
        for e in range(n):
            if f["done"][e, 0]:  # the next step resets whatever the action: start a plain delivery after it
                progs[e] = []
                sub[e] = 0
                continue
            x, y, s, d = (int(v) for v in taxi_decode(int(f["obs"][e, 0])))
            if not progs[e]:
                progs[e] = [("fetch",), ("deliver",)] if s < 4 else [("deliver",)]
            task = progs[e][0]
            if task[0] == "at":
                mv = taxi_toward(x, y, task[1], task[2])
                if mv is None:
                    mv = task[3]
                    progs[e].pop(0)
            elif task[0] == "fetch":
                mv = taxi_toward(x, y, *TAXI_LOC[s]) if s < 4 else 4
                if mv is None:
                    mv = 4
                    progs[e].pop(0)
                elif s == 4:
                    progs[e].pop(0)
            elif task[0] == "deliver":
                mv = taxi_toward(x, y, *TAXI_LOC[d])
                if mv is None:
                    mv = 5
                    progs[e].pop(0)
            else:  # wrong
                depot = (d + 1) % 4
                mv = taxi_toward(x, y, *TAXI_LOC[depot])
                if mv is None:
                    mv = 5 if sub[e] == 0 else 4
                    sub[e] += 1
                    if sub[e] == 2:
                        progs[e].pop(0)
                        sub[e] = 0
            a[e] = mv
        return a
    return policy


def nchain_hold(n):
    return lambda t, f: np.zeros(n, dtype=np.int32)


LAKE4 = ("SFFF", "FHFH", "FFFH", "HFFG")
LAKE8 = ("SFFFFFFF", "FFFFFFFF", "FFFHFFFF", "FFFFFHFF", "FFFHFFFF", "FHHFFFHF", "FHFFHFHF", "FFFHFFFG")
_LAKE_MOVE = ((0, -1), (1, 0), (0, 1), (-1, 0))  # action -> (dx, dy): 0 left, 1 down, 2 right, 3 up


def lake_policy_table(lake):
    """Greedy policy of value iteration under the true dynamics (the action slips to a neighbour with 1/3 each)."""
    size = len(lake)

    def nxt(x, y, a):
        dx, dy = _LAKE_MOVE[a]
        return min(max(x + dx, 0), size - 1), min(max(y + dy, 0), size - 1)

    v = np.zeros((size, size))
    q = np.zeros((size, size, 4))
    for _ in range(400):
        for x in range(size):
            for y in range(size):
                if lake[x][y] in "HG":
                    continue
                for a in range(4):
                    tot = 0.0
                    for slip in (-1, 0, 1):
                        nx, ny = nxt(x, y, (a + slip) % 4)
                        tot += (1.0 if lake[nx][ny] == "G" else 0.999 * v[nx, ny]) / 3.0
                    q[x, y, a] = tot
        v = q.max(axis=2)
    return q.argmax(axis=2).astype(np.int32)


def frozenlake_goal(lake):
    def make(n):
        table = lake_policy_table(lake).reshape(-1)
        size = len(lake)
        odd = np.arange(n) % 2 == 1

        def policy(t, f):  # odd envs head straight down, then right, whatever lies on the way
            obs = f["obs"][:, 0]
            return np.where(odd, np.where(obs // size < size - 1, 1, 2), table[obs]).astype(np.int32)
        return policy
    return make


# ---------------------------------------------------------------------------------------------------------------
# events: name -> predicate(g) -> bool array or count; g maps "actions", "state/<key>" to arrays [T(+1), N, ...]
# ---------------------------------------------------------------------------------------------------------------
def _k(g, key):
    a = np.asarray(g["state/" + key])
    return a.reshape(a.shape[0], a.shape[1], -1)


def _ended(g):  # done, not by the step limit
    return _k(g, "done")[:, :, 0] & ~_k(g, "trunc")[:, :, 0]


def _mc_events(goal, reward=None):
    ev = {
        "goal termination": lambda g: _ended(g) & (_k(g, "obs")[:, :, 0] >= F32(goal)) & (_k(g, "obs")[:, :, 1] >= 0),
        "at the wall with vel zeroed": lambda g: (_k(g, "obs")[:, :, 0] == F32(-1.2)) & (_k(g, "obs")[:, :, 1] == 0),
    }
    if reward is not None:
        ev["reward 100 - 0.1 a^2"] = lambda g: _ended(g) & (_k(g, "reward")[:, :, 0] == F32(reward))
        ev["action clipped on both sides"] = lambda g: min((g["actions"] > 1).sum(), (g["actions"] < -1).sum())
    return ev


def _pendulum_events():
    return {
        "speed clamp +8": lambda g: _k(g, "obs")[:, :, 2] == 8,
        "speed clamp -8": lambda g: _k(g, "obs")[:, :, 2] == -8,
        "torque clipped above": lambda g: g["actions"] > 2,
        "torque clipped below": lambda g: g["actions"] < -2,
        "torque inside the limits": lambda g: np.abs(g["actions"]) < 2,
    }


def _taxi_before_after(g):
    obs = _k(g, "obs")[:, :, 0]
    stepped = _k(g, "elapsed_step")[1:, :, 0] > 0  # row t + 1 is a step of row t, not a reset
    return obs[:-1], g["actions"].reshape(obs[:-1].shape), obs[1:], _k(g, "reward")[1:, :, 0], stepped


def _taxi_blocked_moves(g):
    """Every blocked (cell, move) pair is tried, and leaves the observation as it was."""
    before, act, after, _, stepped = _taxi_before_after(g)
    x, y, _, _ = taxi_decode(before)
    table = np.zeros((5, 5, 4), dtype=bool)
    for m in TAXI_BLOCKED:
        table[m] = True
    blocked = stepped & (act < 4) & table[x, y, np.minimum(act, 3)]
    seen = {(int(a), int(b), int(c)) for a, b, c in zip(x[blocked], y[blocked], act[blocked])}
    return bool((before == after)[blocked].all() and seen == set(TAXI_BLOCKED))


def _taxi_event(select):
    def ev(g):
        before, act, after, rew, stepped = _taxi_before_after(g)
        x, y, s, d = taxi_decode(before)
        at_pass = np.zeros_like(stepped)
        at_dest = np.zeros_like(stepped)
        depot = np.full(before.shape, -1)
        for i, (lx, ly) in enumerate(TAXI_LOC):
            at_pass |= (s == i) & (x == lx) & (y == ly)
            at_dest |= (d == i) & (x == lx) & (y == ly)
            depot = np.where((x == lx) & (y == ly), i, depot)
        return stepped & select(dict(act=act, s=s, after_s=taxi_decode(after)[2], rew=rew, at_pass=at_pass,
                                     at_dest=at_dest, depot=depot, cell=x * 5 + y))
    return ev


def _taxi_events():
    carrying_cells = _taxi_event(lambda v: (v["act"] == 4) & (v["s"] == 4) & (v["rew"] == -10))

    def every_cell(g):
        before, _, _, _, _ = _taxi_before_after(g)
        x, y, _, _ = taxi_decode(before)
        return len(set((x * 5 + y)[carrying_cells(g)].tolist())) == 25
    return {
        "pickup": _taxi_event(lambda v: (v["act"] == 4) & v["at_pass"] & (v["after_s"] == 4) & (v["rew"] == -1)),
        "pickup away from the passenger": _taxi_event(
            lambda v: (v["act"] == 4) & (v["s"] < 4) & ~v["at_pass"] & (v["rew"] == -10)),
        "pickup while carrying at every cell": every_cell,
        "drop-off at the destination": lambda g: _ended(g)[1:] & _taxi_event(
            lambda v: (v["act"] == 5) & (v["s"] == 4) & v["at_dest"] & (v["rew"] == 20))(g),
        "drop-off with an empty taxi": _taxi_event(lambda v: (v["act"] == 5) & (v["s"] < 4) & (v["rew"] == -10)),
        "drop-off at another depot": _taxi_event(
            lambda v: (v["act"] == 5) & (v["s"] == 4) & ~v["at_dest"] & (v["depot"] >= 0) &
            (v["after_s"] == v["depot"]) & (v["rew"] == -1)),
        "drop-off away from any depot": _taxi_event(
            lambda v: (v["act"] == 5) & (v["s"] == 4) & (v["depot"] < 0) & (v["rew"] == -10)),
        "every wall segment and border": _taxi_blocked_moves,
    }


def _lake_events(goal_cell):
    return {
        "goal": lambda g: _ended(g) & (_k(g, "obs")[:, :, 0] == goal_cell) & (_k(g, "reward")[:, :, 0] == 1),
        "hole": lambda g: _ended(g) & (_k(g, "obs")[:, :, 0] != goal_cell) & (_k(g, "reward")[:, :, 0] == 0),
    }


PI4 = F32(4 * np.pi)
THETA_THRESHOLD = 12 * 2 * np.pi / 360

# name -> task, max_steps, extra, T, policy factory, events
SCRIPTED = {
    "mountaincar_pump": dict(task="MountainCar", max_steps=200, extra=(), T=400, policy=mountaincar_pump,
                             events=_mc_events(0.5)),
    "mountaincar_wall": dict(task="MountainCar", max_steps=100000, extra=(), T=400, policy=mountaincar_wall,
                             events={**_mc_events(0.5),
                                     "many wall hits": lambda g: ((_k(g, "obs")[:, :, 0] == F32(-1.2)).sum() >= 20),
                                     "speed clamp -0.07": lambda g: _k(g, "obs")[:, :, 1] == F32(-0.07),
                                     "never truncated": lambda g: not _k(g, "trunc").any()}),
    "mountaincarcont_pump": dict(task="MountainCarContinuous", max_steps=999, extra=(), T=400,
                                 policy=mountaincarcont_pump, events=_mc_events(0.45, 100 - 0.1 * 1.5 * 1.5)),
    "cartpole_drift": dict(task="CartPole", max_steps=500, extra=(), T=500, policy=cartpole_drift, events={
        "x above 2.4, pole upright": lambda g: _ended(g) & (_k(g, "obs")[:, :, 0] > 2.4) &
        (np.abs(_k(g, "obs")[:, :, 2]) < 0.9 * THETA_THRESHOLD),
        "x below -2.4, pole upright": lambda g: _ended(g) & (_k(g, "obs")[:, :, 0] < -2.4) &
        (np.abs(_k(g, "obs")[:, :, 2]) < 0.9 * THETA_THRESHOLD),
    }),
    "acrobot_pump": dict(task="Acrobot", max_steps=100000, extra=(), T=500, policy=acrobot_pump, events={
        "termination with reward 0": lambda g: _ended(g) & (_k(g, "reward")[:, :, 0] == 0),
        "d(theta1) clamped at 4 pi": lambda g: np.abs(_k(g, "obs")[:, :, 4]) == PI4,
    }),
    "pendulum_v0_spin": dict(task="Pendulum", max_steps=200, extra=(0,), T=400, policy=pendulum_spin,
                             events=_pendulum_events()),
    "pendulum_v1_spin": dict(task="Pendulum", max_steps=200, extra=(1,), T=400, policy=pendulum_spin,
                             events=_pendulum_events()),
    "cliffwalking_paths": dict(task="CliffWalking", max_steps=0, extra=(0,), T=120, policy=cliffwalking_paths, events={
        "goal cell 47 with done": lambda g: _k(g, "done")[:, :, 0] & (_k(g, "obs")[:, :, 0] == 47),
        "cliff at every column": lambda g: len(set(
            (_k(g, "obs")[:-1, :, 0] % 12)[(_k(g, "reward")[1:, :, 0] == -100)].tolist())) == 10,
        "right half of the grid": lambda g: _k(g, "obs")[:, :, 0] % 12 >= 6,
    }),
    "cliffwalking_slippery": dict(task="CliffWalking", max_steps=0, extra=(1,), T=300, policy=cliffwalking_slippery,
                                  events={
        "goal cell 47 with done": lambda g: _k(g, "done")[:, :, 0] & (_k(g, "obs")[:, :, 0] == 47),
        "a slip": lambda g: (_k(g, "obs")[:-1, :, 0] // 12 == 0) & (_k(g, "obs")[1:, :, 0] // 12 == 1) &
        (g["actions"].reshape(g["actions"].shape[0], -1) == 1),
    }),
    "taxi_script": dict(task="Taxi", max_steps=200, extra=(), T=400, policy=taxi_script, events=_taxi_events()),
    "nchain_hold": dict(task="NChain", max_steps=1000, extra=(), T=400, policy=nchain_hold, events={
        "reward 10": lambda g: _k(g, "reward")[:, :, 0] == 10,
        "slip: reward 2 under action 0": lambda g: _k(g, "reward")[:, :, 0] == 2,
        "state 4": lambda g: _k(g, "obs")[:, :, 0] == 4,
    }),
    "frozenlake_goal": dict(task="FrozenLake", max_steps=100, extra=(4,), T=400, policy=frozenlake_goal(LAKE4),
                            events=_lake_events(15)),
    "frozenlake8x8_goal": dict(task="FrozenLake", max_steps=200, extra=(8,), T=500, policy=frozenlake_goal(LAKE8),
                               events=_lake_events(63)),
}

SCRIPTED_CLASSIC = sorted(k for k, c in SCRIPTED.items()
                          if c["task"] in ("CartPole", "Pendulum", "MountainCar", "MountainCarContinuous", "Acrobot"))
SCRIPTED_TOY = sorted(set(SCRIPTED) - set(SCRIPTED_CLASSIC))


def rollout(pool, case, n, follower=None):
    """Closed loop: the policy sees `pool`'s frames.  Returns the fixture dict (without the seed); a `follower`
    pool gets the same actions and its frames are returned as a second dict."""
    policy = case["policy"](n)
    frames = [pool.reset()]
    other = [follower.reset()] if follower is not None else None
    actions = []
    for t in range(case["T"]):
        a = policy(t, frames[-1])
        actions.append(a)
        frames.append(pool.step(a))
        if follower is not None:
            other.append(follower.step(a))

    def pack(fr):
        out = {"actions": np.stack(actions)}
        for k in fr[0]:
            out["state/" + k] = np.stack([f[k] for f in fr])
        return out
    return (pack(frames), pack(other)) if follower is not None else pack(frames)


def check_events(name, g):
    """Every event of the case occurs in g (a True, or a count of at least one); returns the counts."""
    counts = {}
    for ev, pred in SCRIPTED[name]["events"].items():
        counts[ev] = int(np.sum(pred(g)))
        assert counts[ev] >= 1, f"scripted_{name}: event '{ev}' is not in the rollout"
    return counts
