"""EnvPoolMixin: send / recv / step / reset / async_reset on top of the native
pool's `_send / _recv / _reset`.

Host-side mirror of envpool/python/envpool.py:61-384 (same method names,
argument meaning and error behaviour).  `render` keeps the reference's checks and
env id forms; the frames come from the pool's render kernel (Jumanji, PGX), and a
family without one surfaces the pool's RuntimeError.
"""

from __future__ import annotations

import pprint
import warnings
from abc import ABC
from typing import Any, NamedTuple

import numpy as np

from envpool_amd.core import native


class Playout(NamedTuple):
    """What `playout` returns: numpy arrays over [k listed envs, R repeats]."""

    returns: np.ndarray  # float32 [k, R, 2]: per-player sum of the step rewards
    plies: np.ndarray    # int32 [k, R]: plies played
    status: np.ndarray   # uint8 [k, R]: 0 the game is over, 1 stopped at max_plies


class Search(NamedTuple):
    """What `search` returns: numpy arrays over [k listed envs, A actions]."""

    visits: np.ndarray   # int32 [k, A]: simulations through each root action
    returns: np.ndarray  # int32 [k, A]: summed playout returns through it, seen from the root's mover
    action: np.ndarray   # int32 [k]: the most visited action (the lowest on ties); -1: the env is over


class Solve(NamedTuple):
    """What `solve` returns: numpy arrays over [k listed envs, A actions]; exact values, seen from the root's mover."""

    value: np.ndarray   # int8 [k]: +1 a forced win, 0, -1 a forced loss (within the horizon); 0 unless status is 0
    q: np.ndarray       # int8 [k, A]: the value through each legal root action; -128: illegal, or status is not 0
    action: np.ndarray  # int32 [k]: the lowest action whose q equals value; -1 unless status is 0
    status: np.ndarray  # uint8 [k]: 0 solved, 1 given up (max_nodes), 2 the env is over
    nodes: np.ndarray   # int64 [k]: the positions visited


class GuidedResult(NamedTuple):
    """What a guided search returns: numpy arrays over [k listed envs, A actions]."""

    visits: np.ndarray  # int32 [k, A]: simulations through each root action
    values: np.ndarray  # float32 [k, A]: summed leaf values through it, seen from the root's mover
    action: np.ndarray  # int32 [k]: the most visited legal action (the lowest on ties); -1: the env was over


class Proof(NamedTuple):
    """What `GuidedSearch.proof` returns: the proven values of a session opened with `prove=True`, seen from the root's
    mover; -128: none."""

    value: np.ndarray  # int8 [k]: the root's proven value, +1, 0 or -1; -128: unproven, or the env was over
    q: np.ndarray      # int8 [k, A]: the proven value of the child of each legal root action; -128: unproven, no child,
                       # illegal (the convention of `Solve.q`)


class Samples(NamedTuple):
    """What `Recorder.drain` returns: numpy arrays over the n training samples written since the last drain."""

    obs: np.ndarray     # bool [n, H, W, C]: the observation of the seat to move
    mask: np.ndarray    # bool [n, A]: the position's legal actions
    policy: np.ndarray  # float32 [n, A]: the policy target given to `add`, 0 on illegal actions and non-finite entries
    value: np.ndarray   # float32 [n]: the game's last reward for the seat that moved at the sample
    ply: np.ndarray     # int32 [n]: the position's elapsed step
    env_id: np.ndarray  # int32 [n]: the env that played the game (global id)
    sym: np.ndarray     # uint8 [n]: the board symmetry of the sample, 0: the identity


class Recorder:
    """A pool's self-play recorder (`env.recorder`): it stages every env's positions and policy targets while its game
    runs, and when a game ends it writes one training sample per staged ply -- with `symmetries=True` one per ply and
    board symmetry -- into a sample buffer on the device, in a deterministic order.

        rec = env.recorder(capacity=1 << 18, symmetries=True)
        ...
        rec.add(result.weights)                    # before the step: the positions as they stand
        _, rew, term, trunc, info = env.step(action)
        rec.finish(rew, term | trunc)              # after it: the games that ended become samples
        s = rec.drain()                            # Samples(obs, mask, policy, value, ply, env_id, sym); count back to 0

    A game that does not fit into the remaining capacity is dropped whole and counted; so is a game whose env was reset
    or restored mid-way (`counters`).  A pool has one recorder; a new one replaces it."""

    def __init__(self, pool: Any, all_ids: np.ndarray, capacity: int, max_plies: int, symmetries: bool) -> None:
        self._pool, self._all = pool, all_ids
        self.shape = pool.record_begin(capacity, max_plies, symmetries)
        self.capacity = int(capacity)

    def _open(self) -> Any:
        if self._pool is None:
            raise ValueError("recorder: the recorder is closed")
        return self._pool

    def _ids(self, env_ids: Any) -> np.ndarray:
        return self._all if env_ids is None else _normalize_env_id(env_ids)

    @property
    def symmetries(self) -> int:
        """Samples per staged ply: 1, or the number of the game's board symmetries."""
        return int(self.shape[4])

    def add(self, policy: Any, env_ids: Any = None) -> None:
        """Before the step: stages the position of every listed env (global ids that do not repeat; None: all) with row
        i of `policy` float32 [k, A] as its target.  Envs whose game is over are skipped."""
        self._open().record_add(policy, self._ids(env_ids))

    def finish(self, reward: Any, done: Any, env_ids: Any = None) -> None:
        """After the step, with what it returned for the listed envs: reward [k, 2] and done [k] (terminated |
        truncated).  The games that ended become samples, in the call's row order."""
        self._open().record_finish(reward, done, self._ids(env_ids))

    def drain(self) -> Samples:
        return Samples(*self._open().record_drain())

    def discard(self, env_ids: Any = None) -> None:
        """Forgets the staged plies of the listed envs (None: of all)."""
        self._open().record_discard(None if env_ids is None else _normalize_env_id(env_ids))

    @property
    def counters(self) -> dict[str, int]:
        """samples and games written, dropped_games and dropped_plies since the recorder was opened."""
        c = self._open().record_counters()
        return dict(samples=int(c[1]), games=int(c[2]), dropped_games=int(c[3]), dropped_plies=int(c[4]))

    def __len__(self) -> int:
        return int(self._open().record_counters()[0])

    def close(self) -> None:
        if self._pool is not None:
            self._pool.record_end()
            self._pool = None


class Rollout(NamedTuple):
    """`ro.batch()`: the collected steps, time-major, rows in env id order.  `obs` has t + 1 slots -- slot s + 1 is the
    observation step s returned --, an array for a single obs key and a dict by state key name for several; the others
    have t rows.  `mask[s, n]` is False where step s was the auto-reset step after a done: slot s then holds the final
    observation of the episode before, the action was ignored and the reward is 0.  With an actor attached
    (`ro.attach`) `logp` [t, N] is the log-probability of each collected action and `value` [t + 1, N] the critic's
    value of every obs slot, both float32; without one they are None."""

    obs: Any
    action: np.ndarray
    reward: np.ndarray
    term: np.ndarray
    trunc: np.ndarray
    mask: np.ndarray
    logp: Any = None
    value: Any = None


class Episodes(NamedTuple):
    """`ro.episodes()`: the episodes finished since the last call, in (step, env id) order: the global env id, the
    collector's step counter at the step that ended it, the float64 sum of its float32 rewards, its length."""

    env_id: np.ndarray
    step: np.ndarray
    ret: np.ndarray
    length: np.ndarray


class RolloutCollector:
    """A pool's rollout collector (`env.rollout`): the pool's own step writes observations, actions, rewards and flags
    time-major into device memory, keeps episode returns and lengths across auto-resets and, with `moments`, float64
    power sums of the observations; `gae` computes advantages on the device (csrc/rollout.hip.h is the contract).

        ro = env.rollout(horizon=128, episodes=1 << 16, moments=True)
        obs, info = ro.reset()
        for t in range(128):
            obs, rew, term, trunc, info = ro.step(policy(obs))     # what env.step returns
        b = ro.batch(); adv, ret = ro.gae(values, 0.99, 0.95); eps = ro.episodes(); ro.next()

    While a collector is open the pool is driven through it: `env.reset` raises ValueError.  `moments()` returns raw
    power sums (count, sum, sum of squares per observation component): mean = sum / count and var = sumsq / count -
    mean^2 are the caller's to derive, and that difference cancels badly where mean^2 is much larger than the variance
    -- centre such observations first.  A pool has one collector; a new one replaces it."""

    def __init__(self, env: Any, pool: Any, horizon: int, episodes: int, moments: bool) -> None:
        self._env, self._pool, self.horizon = env, pool, horizon
        pool.rollout_begin(horizon, episodes, moments)
        self._names = [pool.state_keys[i][0] for i in pool.rollout_obs_keys()]
        self._actor: Any = None

    def _open(self) -> Any:
        if self._pool is None:
            raise ValueError("rollout: the collector is closed")
        return self._pool

    def reset(self) -> Any:
        """What `env.reset()` returns; the observations also land in slot 0, t = 0, and an episode under way is
        abandoned."""
        return self._env._to(self._open().rollout_reset(), True, self._env.config["gym_reset_return_info"])

    def step(self, action: Any) -> Any:
        """What `env.step(action)` returns, bit for bit, for the whole pool in env id order."""
        pool = self._open()
        converted = self._env._from(action)
        self._env._check_action(converted)
        return self._env._to(pool.rollout_step(converted[-1]), False, True)

    @property
    def t(self) -> int:
        return self._open().rollout_shape()[3]

    def batch(self) -> Rollout:
        b, t = self._open().rollout_batch(), self.t
        obs = {n: b[n][:t + 1] for n in self._names}
        logp = value = None
        if self._actor is not None:
            logp, value = self._open().actor_batch()
            logp, value = logp[:t], value[:t + 1]
        return Rollout(obs[self._names[0]] if len(obs) == 1 else obs, b["action"][:t], b["reward"][:t],
                       b["term"][:t].view(np.bool_), b["trunc"][:t].view(np.bool_), b["mask"][:t].view(np.bool_),
                       logp, value)

    def gae(self, values: Any = None, gamma: float = 0.99, lam: float = 0.95) -> tuple[np.ndarray, np.ndarray]:
        """(advantages, returns) float32 [T, N] of a full horizon from `values` float32 [T + 1, N]: a terminated step
        does not bootstrap, a truncated one bootstraps from values[t + 1] (the final observation's) and ends the
        recurrence, a masked step has advantage 0.  With an actor attached `values` may be omitted: the values the
        actor stored are used where they lie."""
        if values is None:
            if self._actor is None:
                raise ValueError("rollout gae: values may only be omitted with an actor attached")
            return self._open().rollout_gae_stored(gamma, lam)
        return self._open().rollout_gae(values, gamma, lam)

    def attach(self, actor: Any, seed: int = 0, deterministic: bool = False) -> None:
        """Attaches an `envpool_amd.actor.Actor`: `collect` then plays with it, `batch()` has `logp` and `value`, and
        `gae()` may use the stored values.  A draw depends on (seed, global env id, the collector's step counter,
        component) only; `deterministic` takes the mode of the policy.  ValueError for an actor of another F, H or
        kind than the pool's.  A new actor replaces the one before; closing the collector releases it."""
        from envpool_amd.actor import space_of

        pool = self._open()
        want = space_of(self._env)
        if (actor.features, actor.actions, actor.kind) != (want["features"], want["actions"], want["kind"]):
            raise ValueError(f"actor: an actor of F = {actor.features}, H = {actor.actions}, kind = {actor.kind} for a "
                             f"pool of F = {want['features']}, H = {want['actions']}, kind = {want['kind']}")
        pool.actor_begin(actor, seed, deterministic, want["actions"])
        self._actor = actor

    def collect(self, steps: Any = None) -> None:
        """Plays `steps` steps (None: the rest of the horizon) with the attached actor, enqueued from C++ with no
        Python, torch or host wait between the launches, and waits for the last one.  `collect(a)` then `collect(b)`
        is `collect(a + b)`; ValueError without an actor, before `reset`, and when the horizon is full."""
        if self._actor is None:
            raise ValueError("rollout collect: the collector has no actor (attach one)")
        if steps is not None and (isinstance(steps, (bool, np.bool_)) or not isinstance(steps, (int, np.integer))
                                  or int(steps) < 1):
            raise ValueError(f"rollout collect: steps = {steps!r} must be None or an integer of at least 1")
        self._open().rollout_collect(0 if steps is None else int(steps))

    def actor_eval(self, obs: Any, env_ids: Any = None, step: Any = None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(action, logp, value) of the attached actor on caller observations (the array of a single obs key, or a dict
        by state key name) for `env_ids` (default: the pool's, in order) at the step counter `step` (default: the
        collector's): what `collect` would compute for these rows.  Nothing of the pool changes."""
        if self._actor is None:
            raise ValueError("rollout actor_eval: the collector has no actor (attach one)")
        pool = self._open()
        arrays = [obs[n] for n in self._names] if isinstance(obs, dict) else [np.asarray(obs)]
        if env_ids is None:
            env_ids = self._env.all_env_ids
        if step is None:
            step = self.counters["steps"]
        return pool.actor_eval(arrays, env_ids, int(step))

    def episodes(self) -> Episodes:
        return Episodes(*self._open().rollout_episodes())

    @property
    def counters(self) -> dict[str, int]:
        """episode rows waiting, episodes finished and dropped (the buffer was full) since the collector was opened,
        and the step counter."""
        c = self._open().rollout_counters()
        return {"count": int(c[0]), "finished": int(c[1]), "dropped": int(c[2]), "steps": int(c[3])}

    def moments(self) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(count, sum, sumsq), float64 per component of the float obs keys (in key order, flattened), over every row
        written into an obs slot by `reset()` and `step()`: raw power sums (see the class docstring)."""
        m = self._open().rollout_moments()
        return m[0], m[1], m[2]

    def next(self) -> None:
        """Slot t becomes slot 0 and t = 0; flags carried over, episode accumulators, episodes and moments are kept."""
        self._open().rollout_next()

    def close(self) -> None:
        pool, self._pool = self._pool, None
        if pool is not None:
            pool.rollout_end()


class Stats(NamedTuple):
    """What a self-play driver has played since it was opened (`Selfplay.run`, `Selfplay.stats`)."""

    games: int   # finished games
    wins0: int   # ... whose last reward was positive for seat 0
    wins1: int   # ... for seat 1
    draws: int   # ... with both rewards 0
    plies: int   # the sum of the finished games' lengths (elapsed steps)
    t: int       # the driver's ply counter: plies played per env, resets included


class Selfplay:
    """A pool's self-play driver (`env.selfplay`): one call plays n plies of every env against itself -- root noise,
    search round with the built-in network, move, recorder add, step with auto-reset, recorder finish, statistics --
    enqueued from C++, with nothing leaving the device between two plies.

        rec = env.recorder(capacity=1 << 18, symmetries=True)
        env.reset()
        sp = env.selfplay(net, policy="gumbel", simulations=32, max_considered=16, batch=16, seed=0)
        stats = sp.run(plies=200)          # Stats(games, wins0, wins1, draws, plies, t)
        samples = rec.drain()
        sp.close()

    `run(n, wait=False)` only enqueues and returns None; `stats()` waits.  The games depend on (seed, env id, the
    driver's ply counter, the net, the positions) only: `run(3)` then `run(2)` is `run(5)`."""

    def __init__(self, pool: Any, net: Any, options: dict) -> None:
        self._pool = pool
        pool.selfplay_begin(net, **options)

    def _open(self) -> Any:
        if self._pool is None:
            raise ValueError("selfplay: the driver is closed")
        return self._pool

    def run(self, plies: int, wait: bool = True) -> Any:
        self._open().selfplay_run(native.check_selfplay_plies(plies), bool(wait))
        return self.stats() if wait else None

    def stats(self) -> Stats:
        return Stats(*(int(x) for x in self._open().selfplay_stats()))

    def noise(self) -> np.ndarray:
        """float32 [num_envs, A]: the last ply's root noise -- the Dirichlet eta rows of a PUCT driver with
        `dirichlet_alpha` (zeros without it, and before the first ply), the Gumbel rows of a Gumbel driver; waits."""
        return self._open().selfplay_noise()

    def close(self) -> None:
        """Releases the driver's device memory; an open recorder stays open."""
        if self._pool is not None:
            pool, self._pool = self._pool, None
            pool.selfplay_end()


class ArenaStats(NamedTuple):
    """What an arena has played since it was opened (`Arena.run`, `Arena.stats`): `Stats`, and the wins by net.
    `wins_a + wins_b + draws == games`; Elo or confidence arithmetic on them is the caller's."""

    games: int   # finished games
    wins0: int   # ... whose last reward was positive for seat 0
    wins1: int   # ... for seat 1
    draws: int   # ... with both rewards 0
    plies: int   # the sum of the finished games' lengths (elapsed steps)
    wins_a: int  # ... whose last reward was positive for net_a's seat (seat e & 1 of the env with global id e)
    wins_b: int  # ... for net_b's seat
    t: int       # the driver's ply counter: plies played per env, resets included


class Arena:
    """A pool's arena (`env.arena`): the self-play driver with two networks, which play each other in every env --
    `net_a` holds seat 0 of the envs with an even global id and seat 1 of those with an odd one, and the env's reset
    coin decides which seat moves first, so over a pool both nets get both seats and both colours.  A ply's search tree
    is evaluated by the net of the seat to move at its root.

        env.reset()
        arena = env.arena(incumbent, candidate, policy="gumbel", simulations=32, batch=16, seed=0)
        stats = arena.run(plies=200)       # ArenaStats(games, wins0, wins1, draws, plies, wins_a, wins_b, t)
        arena.close()

    Without root noise (Gumbel: `noise=True`, the default; PUCT: `dirichlet_alpha` > 0) or `sample_plies` (PUCT), all
    envs of a pool play one of two games -- the nets are deterministic, and only the seat that moves first differs --, so a match needs one of
    them on.  `run(n, wait=False)` only enqueues and returns None; `stats()` waits.  `run(3)` then `run(2)` is
    `run(5)`."""

    def __init__(self, pool: Any, net_a: Any, net_b: Any, options: dict) -> None:
        self._pool = pool
        pool.arena_begin(net_a, net_b, **options)

    def _open(self) -> Any:
        if self._pool is None:
            raise ValueError("arena: the arena is closed")
        return self._pool

    def run(self, plies: int, wait: bool = True) -> Any:
        self._open().arena_run(native.check_selfplay_plies(plies), bool(wait))
        return self.stats() if wait else None

    def stats(self) -> ArenaStats:
        return ArenaStats(*(int(x) for x in self._open().arena_stats()))

    def close(self) -> None:
        """Releases the arena's device memory; an open recorder stays open."""
        if self._pool is not None:
            pool, self._pool = self._pool, None
            pool.arena_end()


class GuidedSearch:
    """A pool's guided-search session (`env.guided_search`): a PUCT search of every listed env whose tree stays on
    the device and that stops at every new leaf for the caller's priors and value.

        gs = env.guided_search(ids, simulations=64)
        result = gs.run(lambda obs, mask, status: model(obs, mask))     # S + 1 evaluations, then closes

    or step by step: `leaves` -> (obs bool [k, H, W, C] of the seat to move, mask bool [k, A], status uint8 [k]:
    0 evaluate, 1 a finished game (the row is ignored), 2 nothing pending); `advance(priors [k, A], values [k])`
    answers them and fetches the next; `result()` at any time; `close()` releases the device memory.

    Tree reuse over a game: open the session with `nodes=` (room per root, simulations + 1 .. 8192), keep it open with
    `run(evaluate, close=False)`, play the move, and `reroot(actions)` makes the subtree under the played move the tree
    of the next round -- the simulations already evaluated below it are kept:

        gs = env.guided_search(ids, simulations=64, nodes=129)
        while playing:
            result = gs.run(evaluate, close=False)
            env.step(result.action, ids)
            gs.reroot(result.action)

    Several leaves per launch: `width=W` (2 .. 32) gives every root W slots; one advance answers all pending slots and
    descends up to W times per root, the descents steered apart by virtual losses, so a move costs about S / W + 1
    model calls of k W rows instead of S + 1 calls of k rows.  `leaves` then carry a slot axis (obs [k, W, H, Wd, C],
    mask [k, W, A], status [k, W]; a slot of status 2 has nothing pending) and `advance` takes priors [k, W, A] and
    values [k, W], or the same flattened to k W rows.  The round is over when `done` is true; `run` flattens the rows
    for `evaluate` -- which therefore is the function written for the plain session -- and loops until then:

        gs = env.guided_search(ids, simulations=64, nodes=129, width=8)
        while playing:
            result = gs.run(evaluate, close=False)      # about 9 model calls of 8 k rows, not 65 of k
            env.step(result.action, ids)
            gs.reroot(result.action)

    Exact leaf status: `tactics=D` (1 .. 16) solves every new leaf other than the root D plies deep (the solver of
    `env.solve`, at most `tactics_nodes` positions per leaf) after the advance's descents.  A leaf that is a forced win
    or loss within D plies needs no evaluation: it comes back with status 1 and zero rows, whatever `advance` is given
    for it is ignored, and the exact +-1 is backed up from then on, as for a finished game.  Every other leaf is
    evaluated as before.  `decided` counts such leaves per root.  After `reroot` onto a decided position the game runs
    on: the new root is handed out for evaluation like any other.

    Proven values: `prove=True` (MCTS-Solver) lets exact values climb the tree.  Finished games and decided leaves are
    proven; a node with a move to a position proven lost for the opponent is proven won, and a node whose every move
    leads to a proven position is proven with the best of them.  A proven node counts as a finished game from then on,
    no descent takes a move proven to lose while another is left, a root that is proven ends its round early (its
    rows have status 2; `run` just goes on for the others), and `result().action` is the most visited move that keeps
    the proven value -- never a move proven to lose while another is not.  `proof` reads the proofs at any time.  With
    `tactics=` the decided leaves feed the proofs, without it only finished games do:

        gs = env.guided_search(ids, simulations=64, tactics=2, prove=True)
        result = gs.run(evaluate, close=False)
        won = gs.proof.value == 1                       # roots with a forced win; result.action plays it"""

    def __init__(self, pool: Any, ids: np.ndarray, simulations: int, c_puct: float, nodes: Any = None,
                 width: int = 1, tactics: int = 0, tactics_nodes: int = native.GUIDED_TACTICS_NODES,
                 prove: bool = False):
        self._pool = pool
        self.simulations = int(simulations)
        self.calls = 0
        self.width = int(width)
        self.tactics = int(tactics)
        self.prove = bool(prove)
        if self.prove:
            self.leaves = pool.guided_begin(ids, int(simulations), float(c_puct), int(nodes or 0),
                                            self.width if self.width > 1 else None, self.tactics, int(tactics_nodes),
                                            True)
        elif self.tactics:
            self.leaves = pool.guided_begin(ids, int(simulations), float(c_puct), int(nodes or 0),
                                            self.width if self.width > 1 else None, self.tactics, int(tactics_nodes))
        elif self.width > 1:
            self.leaves = pool.guided_begin(ids, int(simulations), float(c_puct), int(nodes or 0), self.width)
        elif nodes is None:
            self.leaves = pool.guided_begin(ids, int(simulations), float(c_puct))
        else:
            self.leaves = pool.guided_begin(ids, int(simulations), float(c_puct), int(nodes))

    @property
    def done(self) -> bool:
        """Whether the round is complete: nothing is pending, all statuses are 2."""
        return bool((np.asarray(self.leaves[2]) == 2).all())

    @property
    def decided(self) -> np.ndarray:
        """int32 [k]: the leaves the exact leaf status (`tactics=`) decided per root since the session began; a reroot
        does not reduce it.  Zeros without `tactics`."""
        if self._pool is None:
            raise ValueError("guided search: the session is closed")
        return self._pool.guided_decided()

    @property
    def proof(self) -> Proof:
        """The proven values (`prove=True`) of the roots and of the children of their actions, at any time; -128
        everywhere without `prove`."""
        if self._pool is None:
            raise ValueError("guided search: the session is closed")
        return Proof(*self._pool.guided_proof())

    def advance(self, priors: Any, values: Any) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        if self._pool is None:
            raise ValueError("guided search: the session is closed")
        if self.calls > self.simulations:
            raise ValueError(f"guided_advance: call number {self.calls} is above simulations = {self.simulations}")
        self.leaves = self._pool.guided_advance(priors, values)
        self.calls += 1
        return self.leaves

    def result(self) -> GuidedResult:
        if self._pool is None:
            raise ValueError("guided search: the session is closed")
        return GuidedResult(*self._pool.guided_result())

    def reroot(self, actions: Any, simulations: Any = None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """After the round's last advance: the subtree under `actions[i]` (the move played at root i) becomes root
        i's tree, and a new round of `simulations` (None: as the last one) begins with the new roots as `leaves`,
        which are returned.  A move the search never tried gives a fresh tree; a root whose game the move ends is over
        from then on (status 2, result -1 and zeros).  The kept visits count in `result()`."""
        if self._pool is None:
            raise ValueError("guided search: the session is closed")
        if self.width > 1:
            if not self.done:
                raise ValueError(f"guided_reroot: the round is not complete: "
                                 f"{int((np.asarray(self.leaves[2]) != 2).sum())} slots are pending")
        elif self.calls != self.simulations + 1:
            raise ValueError(f"guided_reroot: the round is not complete: {self.calls} of {self.simulations + 1} "
                             f"advances made")
        s2 = self.simulations if simulations is None else int(simulations)
        self.leaves = self._pool.guided_reroot(actions, s2)
        self.simulations, self.calls = s2, 0
        return self.leaves

    def run(self, evaluate: Any, close: bool = True) -> GuidedResult:
        """Calls `evaluate(obs, mask, status) -> (priors, values)` until simulations + 1 advances are made, returns
        the result and closes the session (`close=False`: leaves it open, for `reroot`).  A wide session calls it
        with the rows flattened to [k W, ...] until the round is `done`, at most simulations + 1 times.  `evaluate`
        may be the built-in network (`envpool_amd.pgx.net.Net`): the same round, enqueued from C++ in one call."""
        if getattr(evaluate, "_is_epa_net", False):  # the built-in network: the round is enqueued from C++
            if self._pool is None:
                raise ValueError("guided search: the session is closed")
            self.leaves, made = self._pool.net_run(evaluate, self.leaves)
            self.calls += made
        while self.width > 1 and not self.done and self.calls <= self.simulations:
            obs, mask, status = self.leaves
            self.advance(*evaluate(obs.reshape((-1,) + obs.shape[2:]), mask.reshape(-1, mask.shape[-1]),
                                   status.reshape(-1)))
        while self.width == 1 and self.calls <= self.simulations:
            self.advance(*evaluate(*self.leaves))
        out = self.result()
        if close:
            self.close()
        return out

    def close(self) -> None:
        if self._pool is not None:
            pool, self._pool = self._pool, None
            pool.guided_end()


class GumbelResult(NamedTuple):
    """What a Gumbel search returns: numpy arrays over [k listed envs, A actions]."""

    visits: np.ndarray   # int32 [k, A]: simulations through each root action
    values: np.ndarray   # float32 [k, A]: summed leaf values through it, seen from the root's mover
    action: np.ndarray   # int32 [k]: the recommended move (the best of the most visited); -1: the env was over
    weights: np.ndarray  # float32 [k, A]: the improved policy softmax(logits + sigma(completed q)): the training target


class GumbelSearch:
    """A pool's Gumbel-search session (`env.gumbel_search`): Gumbel top-m sampling with sequential halving at the root
    of every listed env, the tree on the device, stopping at every new leaf for the caller's logits and value.

        gs = env.gumbel_search(ids, simulations=32, max_considered=16, seed=0)
        result = gs.run(lambda obs, mask, status: model(obs, mask))     # S + 1 evaluations, then closes

    or step by step, as `GuidedSearch`: `leaves`, `advance(logits [k, A], values [k])`, `result()`, `close()`.

    A halving level per launch: `batch=B` (2 .. 32) gives every root B slots, and one advance makes up to B simulations
    of the root's current level of sequential halving -- the simulations with the same considered visit count, which
    go through different root actions, so nothing collides and no virtual loss is needed.  The launch scores the root
    once and takes its actions together (the plain session re-scores it before every simulation, so the two differ
    where the values are not constant).  S = 32, m = 16, B = 16 costs 5 model calls of k B rows, not 33 of k.
    `leaves` then carry a slot axis (obs [k, B, H, W, C], mask [k, B, A], status [k, B]; a slot of status 2 has
    nothing pending) and `advance` takes logits [k, B, A] and values [k, B], or the same flattened to k B rows.  The
    round is over when `done` is true; `run` flattens the rows for `evaluate` -- which therefore is the function
    written for the plain session -- and loops until then:

        while playing:
            result = env.gumbel_search(ids, simulations=32, max_considered=16, batch=16).run(evaluate)
            env.step(result.action, ids)"""

    def __init__(self, pool: Any, ids: np.ndarray, simulations: int, max_considered: int, gumbel: np.ndarray,
                 c_visit: float, c_scale: float, batch: int = 1):
        self._pool = pool
        self.simulations = int(simulations)
        self.calls = 0
        self.batch = int(batch)
        if self.batch > 1:
            self.leaves = pool.gumbel_begin(gumbel, ids, int(simulations), int(max_considered), float(c_visit),
                                            float(c_scale), self.batch)
        else:
            self.leaves = pool.gumbel_begin(gumbel, ids, int(simulations), int(max_considered), float(c_visit),
                                            float(c_scale))

    @property
    def done(self) -> bool:
        """Whether the round is complete: nothing is pending, all statuses are 2."""
        return bool((np.asarray(self.leaves[2]) == 2).all())

    def advance(self, logits: Any, values: Any) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        if self._pool is None:
            raise ValueError("gumbel search: the session is closed")
        if self.calls > self.simulations:
            raise ValueError(f"gumbel_advance: call number {self.calls} is above simulations = {self.simulations}")
        self.leaves = self._pool.gumbel_advance(logits, values)
        self.calls += 1
        return self.leaves

    def result(self) -> GumbelResult:
        if self._pool is None:
            raise ValueError("gumbel search: the session is closed")
        return GumbelResult(*self._pool.gumbel_result())

    def run(self, evaluate: Any) -> GumbelResult:
        """Calls `evaluate(obs, mask, status) -> (logits, values)` until simulations + 1 advances are made, returns
        the result and closes the session.  A batch session calls it with the rows flattened to [k B, ...] until the
        round is `done`, at most simulations + 1 times.  `evaluate` may be the built-in network
        (`envpool_amd.pgx.net.Net`): the same round, enqueued from C++ in one call."""
        if getattr(evaluate, "_is_epa_net", False):  # the built-in network: the round is enqueued from C++
            if self._pool is None:
                raise ValueError("gumbel search: the session is closed")
            self.leaves, made = self._pool.net_run(evaluate, self.leaves)
            self.calls += made
        while self.batch > 1 and not self.done and self.calls <= self.simulations:
            obs, mask, status = self.leaves
            self.advance(*evaluate(obs.reshape((-1,) + obs.shape[2:]), mask.reshape(-1, mask.shape[-1]),
                                   status.reshape(-1)))
        while self.batch == 1 and self.calls <= self.simulations:
            self.advance(*evaluate(*self.leaves))
        out = self.result()
        self.close()
        return out

    def close(self) -> None:
        if self._pool is not None:
            pool, self._pool = self._pool, None
            pool.guided_end()


def _normalize_env_id(env_id: Any) -> Any:
    """env ids as an int32 array of at least one dimension (envpool.py:38-48).  Array-likes with their own `astype`
    (device arrays) keep their type; everything else goes through numpy."""
    if hasattr(env_id, "astype"):
        # numpy: no copy when the dtype already matches; other array types: their own conversion
        ids = env_id.astype(np.int32, copy=False) if isinstance(env_id, np.ndarray) else env_id.astype(np.int32)
    else:
        ids = np.asarray(env_id, dtype=np.int32)
    return ids.reshape(1) if getattr(ids, "ndim", 0) == 0 else ids


def _flatten_action_dict(action: dict, prefix: tuple = ()) -> dict[str, Any]:
    """{"a": {"b": x}} -> {"a.b": x} (the reference uses optree paths)."""
    out: dict[str, Any] = {}
    for k, v in action.items():
        if isinstance(v, dict):
            out.update(_flatten_action_dict(v, prefix + (k,)))
        else:
            out[".".join(prefix + (k,))] = v
    return out


class EnvPoolMixin(ABC):
    """Mixin class for EnvPool, exposed to the gymnasium / dm metaclasses."""

    def _check_action(self, actions: list[np.ndarray]) -> None:
        """dtype and per-row shape of every action array against the spec -- on the FIRST send only
        (envpool.py:151-172); the messages are the reference's."""
        if getattr(self, "_check_action_finished", False):
            return
        self._check_action_finished = True
        specs = self.spec.action_array_spec
        for arr, (name, want) in zip(actions, specs.items()):
            if arr.dtype != want.dtype:
                raise RuntimeError(f'Expected dtype {want.dtype} with action "{name}", got {arr.dtype}')
            shape = tuple(want.shape)
            per_player = len(shape) > 0 and shape[0] == -1  # leading -1: one row per player
            if per_player:
                ok, shown = arr.shape[1:] == shape[1:], shape
            else:
                ok, shown = arr.ndim > 0 and arr.shape[1:] == shape, ("num_env", *shape)
            if not ok:
                raise RuntimeError(f'Expected shape {shown} with action "{name}", got {arr.shape}')

    def _from(self, action: dict[str, Any] | np.ndarray,
              env_id: np.ndarray | None = None) -> list[np.ndarray]:
        """Convert an action into the native list (envpool.py:174-208)."""
        if isinstance(action, dict):
            adict = _flatten_action_dict(action)
        else:
            # a bare array is the LAST action key (the other two are the env ids); its dtype comes from the spec
            if not hasattr(self, "_last_action_name"):
                self._last_action_name = self._spec._action_keys[-1]
                self._last_action_type = self._spec._action_spec[-1][0]
            if isinstance(action, np.ndarray):
                # (the reference copies here; the pool stages the rows before `send` returns, so an
                # array that already has the dtype and layout can be passed through)
                action = action.astype(self._last_action_type, order="C", copy=False)
            adict = {self._last_action_name: action}
        if env_id is not None:
            adict["env_id"] = env_id.astype(np.int32, copy=False)
        else:
            adict.setdefault("env_id", self.all_env_ids)
        if "players.env_id" not in adict:
            # one action row per env (every family here): players.env_id == env_id
            adict["players.env_id"] = _normalize_env_id(adict["env_id"])
        if not hasattr(self, "_action_names"):
            self._action_names = self._spec._action_keys
        return [adict[name] for name in self._action_names]

    def __len__(self) -> int:
        return self.config["num_envs"]

    @property
    def all_env_ids(self) -> np.ndarray:
        if not hasattr(self, "_all_env_ids"):
            # `env_id_offset` (extension): this pool is one shard of a bigger pool and
            # its env ids are the global ones [offset, offset + num_envs)
            off = int(self.config.get("env_id_offset", 0))
            self._all_env_ids = np.arange(off, off + self.config["num_envs"], dtype=np.int32)
        return self._all_env_ids

    @property
    def is_async(self) -> bool:
        return (self.config["batch_size"] > 0
                and self.config["num_envs"] != self.config["batch_size"])

    def seed(self, seed: int | list[int] | None = None) -> None:
        warnings.warn(
            "The `seed` function in envpool is abandoned. "
            "You can set seed by envpool.make(..., seed=seed) instead.",
            stacklevel=2,
        )

    def render(self, env_ids: Any = None, camera_id: int | None = None) -> Any:
        render_mode = getattr(self, "_render_mode", None)
        if render_mode not in {"rgb_array", "human"}:
            raise RuntimeError(
                "render_mode must be set to 'rgb_array' or 'human' when creating this env"
            )
        # envpool.py:51-58: None is render_env_id; an int, a list or an array name the envs
        if env_ids is None:
            ids = np.asarray([int(getattr(self, "_render_env_id", 0))], dtype=np.int32)
        elif isinstance(env_ids, (int, np.integer)):
            ids = np.asarray([env_ids], dtype=np.int32)
        else:
            ids = np.asarray(_normalize_env_id(env_ids), dtype=np.int32)
        frames = self._render(
            ids,
            int(getattr(self, "_render_width", 0)),
            int(getattr(self, "_render_height", 0)),
            int(getattr(self, "_render_camera_id", -1) if camera_id is None else camera_id),
        )
        if render_mode == "human":  # envpool.py:288-294 (the window itself needs opencv, which is optional)
            if ids.shape[0] != 1:
                raise ValueError("render_mode='human' only supports a single env_id")
            try:
                import cv2
            except ImportError as exc:
                raise RuntimeError("render_mode='human' requires opencv-python to be installed") from exc
            name = getattr(self, "_render_window_name", f"{self.__class__.__name__}-render")
            cv2.imshow(name, np.ascontiguousarray(frames[0][:, :, ::-1]))
            cv2.waitKey(1)
            self._render_window_name = name
            return None
        return frames

    def snapshot(self, env_ids: Any = None, rng: bool = True) -> Any:
        """Extension: everything that makes the listed envs (global ids; None: all) continue bit for bit, as an opaque
        uint8 blob -- with `rng` their generators too, so that resets and random transitions repeat as well.  A pool
        sharded over several devices returns one blob per shard and takes no `env_ids`."""
        return self._snapshot(None if env_ids is None else _normalize_env_id(env_ids), bool(rng))

    def restore(self, blob: Any, env_ids: Any = None) -> None:
        """Extension: put a `snapshot` (of this pool, or of another pool of the same task and frame_stack) into the
        listed envs; None: envs 0 .. k-1 of this pool, k being the number of envs in the blob."""
        self._restore(blob, None if env_ids is None else _normalize_env_id(env_ids))

    def fork(self, src: Any, dst: Any, rng: bool = True) -> None:
        """Extension: env dst[i] becomes env src[i] without leaving the device (tree search: one position into many
        envs).  `src` may repeat, `dst` must not."""
        self._fork(_normalize_env_id(src), _normalize_env_id(dst), bool(rng))

    def playout(self, env_ids: Any = None, repeats: int = 1, max_plies: int = 0, seed: int = 0,
                commit: bool = False) -> Playout:
        """Extension (the PGX board games): `repeats` uniform-random playouts of every listed env (global ids; None:
        all) from its current position to the end of the game, or for `max_plies` plies (0: 256), in one kernel
        launch -- the leaf evaluation of a tree search.  The picks depend on (seed, env id, repeat, ply) and the
        position only.  Nothing of the pool changes, unless `commit` (repeats = 1, ids that do not repeat) writes the
        final positions back as if the plies had been stepped.  The arguments are checked before any native call."""
        ids = native.check_playout(self.all_env_ids if env_ids is None else _normalize_env_id(env_ids),
                                   repeats, max_plies, commit)
        return Playout(*self._playout(ids, int(repeats), int(max_plies), int(seed), bool(commit)))

    def search(self, env_ids: Any = None, simulations: int = 64, leaf_playouts: int = 8, c_puct: float = 1.25,
               max_plies: int = 0, seed: int = 0) -> Search:
        """Extension (the PGX board games): a tree search from the current position of every listed env (global ids;
        None: all) in one kernel launch -- `simulations` rounds of PUCT selection with uniform priors, every new leaf
        valued by `leaf_playouts` random playouts (`max_plies`, `seed` as for `playout`, whose repeats
        0 .. simulations * leaf_playouts - 1 they are).  The result depends on the arguments, the env id and the
        position only.  Nothing of the pool changes.  The arguments are checked before any native call."""
        ids = native.check_search(self.all_env_ids if env_ids is None else _normalize_env_id(env_ids),
                                  simulations, leaf_playouts, c_puct, max_plies)
        return Search(*self._search(ids, int(simulations), int(leaf_playouts), float(c_puct), int(max_plies),
                                    int(seed)))

    def solve(self, env_ids: Any = None, depth: int = 0, max_nodes: int = 1 << 20, table_bits: int = 0) -> Solve:
        """Extension (the PGX board games): the exact minimax value of the current position of every listed env
        (global ids; None: all), by alpha-beta in one kernel launch; no model, no random numbers.  `depth`: the
        horizon in plies -- value +1 is then a forced win within `depth` plies, -1 a forced loss, 0 neither --, 0: to
        the end of the game.  A root that visits more than `max_nodes` positions is given up (status 1).  Nothing of
        the pool changes.  The arguments are checked before any native call.
        `table_bits` = b, 1 .. 16, gives every lane of a root's wave a private transposition table of 2^b entries
        (32 bytes each, 64 lanes per root) for the call: a position the lane meets again, by another order of the same
        moves, is not searched again.  The values are the same; `nodes` is mostly smaller, so a deep solve that is
        given up at `max_nodes` without tables may be solved with them.  0: no tables."""
        ids = native.check_solve(self.all_env_ids if env_ids is None else _normalize_env_id(env_ids), depth, max_nodes,
                                 table_bits)
        return Solve(*self._solve(ids, int(depth), int(max_nodes), int(table_bits)))

    def evaluate(self, net: Any, env_ids: Any = None, priors: bool = False) -> tuple[np.ndarray, np.ndarray]:
        """Extension (the PGX board games; the other families raise RuntimeError): the built-in network `net`
        (`envpool_amd.pgx.net.Net`) on the current position of every listed env, seen by the seat to move: (policy
        float32 [k, A] -- logits, or with `priors` the softmax over the legal actions --, value float32 [k]); an env
        that is over gets zeros.  Playing `policy.argmax` over the legal actions is a raw-policy move without a
        search.  It opens and closes the pool's guided-search session, so it replaces an open one."""
        pool = self._guided()
        ids = native.check_guided(self.all_env_ids if env_ids is None else _normalize_env_id(env_ids), 1, 0.0)
        leaves = pool.guided_begin(ids, 1, 0.0)
        try:
            return pool.net_eval(net, *leaves, priors)
        finally:
            pool.guided_end()

    def guided_search(self, env_ids: Any = None, simulations: int = 64, c_puct: float = 1.25, policy: str = "puct",
                      nodes: Any = None, width: int = 1, tactics: int = 0,
                      tactics_nodes: int = native.GUIDED_TACTICS_NODES, prove: bool = False, **gumbel: Any) -> Any:
        """Extension (the PGX board games): opens a guided tree search from the current position of every listed env
        (global ids; None: all) -- PUCT selection with the priors and leaf values the caller supplies, one kernel
        launch per simulation, the tree on the device (AlphaZero-style search).  Returns the `GuidedSearch` session; a
        pool has one at a time, and a new one replaces it.  Nothing of the pool changes.  The arguments are checked
        before any native call.  `policy="gumbel"` is `gumbel_search(env_ids, simulations, **gumbel)` instead (c_puct
        is not used; `batch=` among them: a halving level per launch) and returns a `GumbelSearch`.
        `nodes` (PUCT only): the node capacity per root, simulations + 1 ..
        8192 (None: simulations + 1), the room `GuidedSearch.reroot` needs to keep the played move's subtree.  `width`
        (PUCT only), 1 .. 32: the leaves per root and launch (`GuidedSearch`: "Several leaves per launch"); 1 is the
        plain session.  `tactics` (PUCT only), 1 .. 16: the exact leaf status (`GuidedSearch`: "Exact leaf status"),
        every new leaf solved that many plies deep with at most `tactics_nodes` (1 .. 2^20) positions; 0: off.
        `prove` (PUCT only): proven values (`GuidedSearch`: "Proven values"), exact values climb the tree; False:
        off."""
        native.check_guided_width(width)
        tactics, tactics_nodes = native.check_guided_tactics(tactics, tactics_nodes)
        prove = native.check_guided_prove(prove)
        if policy == "gumbel":
            if prove:
                raise ValueError("guided_search: prove is an argument of policy='puct' (proven values not "
                                 "implemented for gumbel sessions)")
            if tactics:
                raise ValueError("guided_search: tactics is an argument of policy='puct' (exact leaf status not "
                                 "implemented for gumbel sessions)")
            if width != 1:
                raise ValueError("guided_search: width is an argument of policy='puct' (several leaves per launch not "
                                 "implemented for gumbel sessions)")
            if nodes is not None:
                raise ValueError("guided_search: nodes is an argument of policy='puct' (reroot not implemented for "
                                 "gumbel sessions)")
            return self.gumbel_search(env_ids, simulations, **gumbel)
        if policy != "puct":
            raise ValueError(f"guided_search: policy = {policy!r} must be 'puct' or 'gumbel'")
        if gumbel:
            raise ValueError(f"guided_search: {sorted(gumbel)} are arguments of policy='gumbel'")
        ids = native.check_guided(self.all_env_ids if env_ids is None else _normalize_env_id(env_ids),
                                  simulations, c_puct)
        if nodes is not None:
            native.check_guided_nodes(simulations, nodes)
        if prove:
            return GuidedSearch(self._guided(), ids, int(simulations), float(c_puct), nodes, int(width), tactics,
                                tactics_nodes, True)
        if tactics:
            return GuidedSearch(self._guided(), ids, int(simulations), float(c_puct), nodes, int(width), tactics,
                                tactics_nodes)
        return GuidedSearch(self._guided(), ids, int(simulations), float(c_puct), nodes, int(width))

    def gumbel_search(self, env_ids: Any = None, simulations: int = 32, max_considered: int = 16, gumbel: Any = None,
                      seed: Any = None, c_visit: float = 50.0, c_scale: float = 0.1,
                      width: int = 1, batch: int = 1, tactics: int = 0, prove: bool = False) -> GumbelSearch:
        """Extension (the PGX board games): opens a Gumbel search (Danihelka et al., ICLR 2022) from the current
        position of every listed env (global ids; None: all): Gumbel top-`max_considered` sampling without replacement
        at the root, sequential halving of the `simulations` over those actions, a deterministic rule inside the tree;
        the caller supplies logits and values at every new leaf.  The result's `action` is the move to play and its
        `weights` the policy training target.  `gumbel` float32 [k, A] is the root noise (zeros: no noise, for
        evaluation); None draws it on the host from numpy.random.Generator(PCG64(seed)), seed=None unseeded.  Returns
        the `GumbelSearch` session; it is the pool's one guided-search session.  Nothing of the pool changes.  The
        arguments are checked before any native call.  `batch`, 1 .. 32: the simulations of a halving level per root
        and launch (`GumbelSearch`: "A halving level per launch"); 1 is the plain session.  `width` other than 1
        raises: it is the virtual-loss rule of the PUCT sessions, and a Gumbel session batches by level instead."""
        if width != 1:
            raise ValueError("gumbel_search: width is an argument of policy='puct' (several leaves per launch not "
                             "implemented for gumbel sessions)")
        if tactics:
            raise ValueError("gumbel_search: tactics is an argument of policy='puct' (exact leaf status not implemented "
                             "for gumbel sessions)")
        if native.check_guided_prove(prove):
            raise ValueError("gumbel_search: prove is an argument of policy='puct' (proven values not implemented for "
                             "gumbel sessions)")
        native.check_gumbel_batch(batch)
        ids = native.check_gumbel(self.all_env_ids if env_ids is None else _normalize_env_id(env_ids),
                                  simulations, max_considered, c_visit, c_scale)
        pool = self._gumbel()
        actions = pool.gumbel_actions()
        if gumbel is None:
            gumbel = np.random.Generator(np.random.PCG64(seed)).gumbel(size=(len(ids), actions)).astype(np.float32)
        gumbel = native.check_gumbel_noise(gumbel, len(ids), actions)
        return GumbelSearch(pool, ids, int(simulations), int(max_considered), gumbel, float(c_visit), float(c_scale),
                            int(batch))

    def recorder(self, capacity: int, max_plies: int = 0, symmetries: bool = False) -> Recorder:
        """Extension (the PGX board games): opens the pool's self-play recorder -- `Recorder`: `add` before every step,
        `finish` after it, and the finished games arrive as training samples (obs of the seat to move, legal mask,
        policy target, the game's result as the value, ply, env id, symmetry) in a device buffer of `capacity` rows,
        which `drain` hands over.  `max_plies`: the plies staged per env, 0 .. 256 (0: 128; no game of the four lasts
        longer than 122).  `symmetries`: every board symmetry of each sample (TicTacToe, Othello: 8; ConnectFour, Hex:
        2).  A pool has one recorder at a time; it coexists with a search session.  The arguments are checked before any
        native call."""
        capacity, max_plies, symmetries = native.check_record(capacity, max_plies, symmetries)
        return Recorder(self._recorder(), np.asarray(self.all_env_ids, dtype=np.int32), capacity, max_plies, symmetries)

    def rollout(self, horizon: int, episodes: int = 0, moments: bool = False) -> RolloutCollector:
        """Extension (every family with one row per env and a device step; the PGX games and Atari raise
        RuntimeError("rollout not implemented for this environment")): opens the pool's rollout collector --
        `RolloutCollector` -- with time-major buffers of `horizon` steps, `episodes` rows for finished episodes and,
        with `moments`, observation power sums.  Sync pools only.  The arguments are checked before any native call."""
        pool = self._rollout()
        if self.is_async:
            raise ValueError("rollout: async mode (batch_size != num_envs) is not supported")
        obs, act = pool.rollout_row_bytes()
        horizon, episodes, moments = native.check_rollout(horizon, episodes, moments, self.config["num_envs"], obs, act)
        return RolloutCollector(self, pool, horizon, episodes, moments)

    def selfplay(self, net: Any, policy: str = "gumbel", simulations: int = 32, seed: int = 0, record: bool = True,
                 **options: Any) -> Selfplay:
        """Extension (the PGX board games): opens the pool's self-play driver -- `Selfplay` -- with the built-in
        network `net` (`envpool_amd.pgx.net.Net`) as the evaluator.  `policy="gumbel"` takes `max_considered`,
        `c_visit`, `c_scale`, `batch` and `noise` (False: zero root noise) as `gumbel_search` does;
        `policy="puct"` takes `c_puct`, `width`, `tactics`, `tactics_nodes`, `prove` as `guided_search` does and
        `sample_plies`: a game's first plies are sampled from the visit counts, the later ones take the most visited
        move.  `policy="puct"` also takes standard AlphaZero exploration: `dirichlet_alpha` > 0 (default 0: none) mixes
        eta ~ Dir(alpha) over the legal root actions into every root's priors, (1 - `dirichlet_eps`) p +
        `dirichlet_eps` eta (default 0.25), before the search expands the root; `temperature` T (default 1, 0.05 .. 20)
        samples the first `sample_plies` plies from visits^(1/T).  The policy target stays visits / sum.
        `record` (default True) feeds the pool's open recorder.  The pool must be in sync mode with nothing
        pending in its result queue (after `reset()` or `step()`).  A `batch` or `width` session reads one device word
        per advance, as `search.run(net)` does; a plain session has no host wait between plies.  The arguments are
        checked before any native call."""
        if not getattr(net, "_is_epa_net", False):
            raise ValueError("selfplay: net must be an envpool_amd.pgx.net.Net")
        options = dict(options, policy=policy, simulations=simulations, seed=seed, record=record)
        native.check_selfplay(**options)
        if self.is_async:
            raise ValueError("selfplay: async mode (batch_size != num_envs) is not supported")
        return Selfplay(self._selfplay(), net, options)

    def evaluate_pair(self, net_a: Any, net_b: Any, side: Any, env_ids: Any = None,
                      priors: bool = False) -> tuple[np.ndarray, np.ndarray]:
        """Extension (the PGX board games): `evaluate` with two networks in one launch -- row i (the current position
        of env_ids[i]) is evaluated by `net_a` where `side[i]` is 0 and by `net_b` where it is 1, and gets exactly what
        `evaluate` of that net gives it.  The nets must agree in inputs and actions; width and depth may differ."""
        native.check_arena(net_a, net_b)
        pool = self._guided()
        ids = native.check_guided(self.all_env_ids if env_ids is None else _normalize_env_id(env_ids), 1, 0.0)
        side = native.check_arena_side(side, len(ids))
        leaves = pool.guided_begin(ids, 1, 0.0)
        try:
            return pool.net_eval_pair(net_a, net_b, *leaves, side, priors)
        finally:
            pool.guided_end()

    def arena(self, net_a: Any, net_b: Any, policy: str = "gumbel", simulations: int = 32, seed: int = 0,
              record: bool = False, **options: Any) -> Arena:
        """Extension (the PGX board games): opens the pool's self-play driver as an arena -- `Arena` -- in which the
        built-in networks `net_a` and `net_b` (`envpool_amd.pgx.net.Net`; the same inputs and actions, any width and
        depth) play each other: `net_a` moves for seat e & 1 of the env with global id e.  The options are those of
        `selfplay`, `dirichlet_alpha`, `dirichlet_eps` and `temperature` included (the same for both nets);
        `record` (default False) feeds the pool's open recorder.  Without root noise (Gumbel; PUCT:
        `dirichlet_alpha`) or `sample_plies` (PUCT), all envs of a pool play one of two games, so a match needs one of
        them on.  The
        arguments are checked before any native call."""
        options = dict(options, policy=policy, simulations=simulations, seed=seed, record=record)
        native.check_arena(net_a, net_b, **options)
        if self.is_async:
            raise ValueError("arena: async mode (batch_size != num_envs) is not supported")
        return Arena(self._selfplay(), net_a, net_b, options)

    def send(self, action: dict[str, Any] | np.ndarray,
             env_id: np.ndarray | None = None) -> None:
        converted_action = self._from(action, env_id)
        self._check_action(converted_action)
        self._send(converted_action)

    def recv(self, reset: bool = False, return_info: bool = True) -> Any:
        state_list = self._recv()
        return self._to(state_list, reset, return_info)

    def async_reset(self) -> None:
        self._reset(self.all_env_ids)

    def step(self, action: dict[str, Any] | np.ndarray,
             env_id: np.ndarray | None = None) -> Any:
        self.send(action, env_id)
        return self.recv(reset=False, return_info=True)

    def reset(self, env_id: np.ndarray | None = None) -> Any:
        if env_id is None:
            env_id = self.all_env_ids
        self._reset(env_id)
        return self.recv(reset=True, return_info=self.config["gym_reset_return_info"])

    def close(self) -> None:
        close = getattr(super(), "close", None)
        if close is not None:
            close()

    @property
    def config(self) -> dict[str, Any]:
        return dict(zip(self._spec._config_keys, self._spec._config_values))

    def __repr__(self) -> str:
        config_str = ", ".join(f"{k}={pprint.pformat(v)}" for k, v in self.config.items())
        return f"{self.__class__.__name__}({config_str})"

    __str__ = __repr__
