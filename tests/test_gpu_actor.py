"""Rollout actor on the device.  `actor_eval` equals the g++ build of csrc/actor.hip.h (tests/cpu_harness/actor_host.cpp)
bit for bit -- the features kernel, the int8 trunk's raw form and the sample kernel in one --; `ro.collect()` equals the
host-driven loop `a, logp, v = actor_eval(obs of slot t); ro.step(a)` on a twin pool with the same seed, byte for byte in
every buffer.  N = 257 is odd and more than one features block (64 rows), net wave (64 rows) and sample block (256)."""
import numpy as np
import pytest

import actor_util as au
import envpool_amd as envpool
from envpool_amd.actor import Actor
from envpool_amd.pgx.net import Net
from test_actor_host import harness_features, lib, vp  # noqa: F401  (lib: the g++ harness, a fixture)

pytestmark = pytest.mark.gpu

N, T = 257, 7
F32 = np.float32
TASKS = {
    "CartPole-v1": dict(max_episode_steps=3),   # masked rows and truncation inside a horizon
    "Pendulum-v1": dict(max_episode_steps=5),
    "Taxi-v3": dict(max_episode_steps=4),
    "MiniGrid-Empty-5x5-v0": dict(max_episode_steps=5),
    "HalfCheetah-v4": dict(max_episode_steps=6),
    "Game2048-v1": dict(max_episode_steps=4),
}
SIGMA = {"Pendulum-v1": 50.0}  # both clamps of [-2, 2] are reached


def same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def make(task, n, seed=7, **kw):
    return envpool.make(task, "gymnasium", num_envs=n, seed=seed, **dict(TASKS[task], **kw))


def actor_for(env, task, seed=2):
    """hidden = 32, one block.  The logits are scaled down by 16, so that no action of a random net wins every draw and
    the noise decides (an untrained net's observations barely differ between envs)."""
    a = Actor.random(env, hidden=32, blocks=1, seed=seed, sigma=SIGMA.get(task, 0.5))
    net = Net(a.net.obs_shape, a.actions, 32, 1, a.net.layers, a.net.scale_p / 16, a.net.scale_v)
    return Actor(net, a.kind, a.lo, a.scale, a.sigma, a.low, a.high)


def open_ro(task, n, actor_seed=9, deterministic=False, horizon=T, moments=True, **kw):
    env = make(task, n, **kw)
    ro = env.rollout(horizon=horizon, episodes=4 * n * horizon, moments=moments)
    actor = actor_for(env, task)
    ro.attach(actor, seed=actor_seed, deterministic=deterministic)
    return env, ro, actor


def obs_list(ro, obs, slot=None):
    """The arrays of one obs slot in key order."""
    arrays = [obs[k] for k in ro._names] if isinstance(obs, dict) else [obs]
    return arrays if slot is None else [a[slot] for a in arrays]


def harness_eval(lib, actor, obs, ids, step, seed, deterministic):
    """(action float32 / int32, logp, value) of the g++ build for the rows `obs` (a list of arrays in key order)."""
    feat = harness_features(lib, [np.ascontiguousarray(o).reshape(len(ids), -1) for o in obs], actor.lo, actor.scale)
    assert np.array_equal(feat, au.features(obs, actor.lo, actor.scale))
    blob = actor.blob()
    h, rows = actor.actions, len(ids)
    p = np.empty((rows, h + 1), np.int32)
    assert lib.ah_head(vp(blob), blob.nbytes, vp(feat), rows, vp(p)) == 1
    ids = np.ascontiguousarray(ids, np.int32)
    logp, value = np.empty(rows, F32), np.empty(rows, F32)
    sp, sv = F32(actor.net.scale_p), F32(actor.net.scale_v)
    if actor.kind == 0:
        action = np.empty(rows, np.int32)
        lib.ah_discrete(vp(p), rows, h, sp, sv, seed, vp(ids), step, int(deterministic), vp(action), vp(logp), vp(value))
    else:
        action = np.empty((rows, h), F32)
        lib.ah_box(vp(p), rows, h, sp, sv, vp(actor.sigma), vp(actor.low), vp(actor.high), seed, vp(ids), step,
                   int(deterministic), vp(action), vp(logp), vp(value))
    return action, logp, value, feat


@pytest.mark.parametrize("task", list(TASKS))
@pytest.mark.parametrize("deterministic", [False, True])
def test_actor_eval_equals_the_host_build(lib, task, deterministic):
    env, ro, actor = open_ro(task, N, actor_seed=2**40 + 5, deterministic=deterministic, env_id_offset=1000)
    ro.reset()
    ro.collect(3)                                     # observations a few steps in, not only reset states
    b = ro.batch()
    obs = obs_list(ro, b.obs, 3)
    ids = env.all_env_ids[::-1].copy()                # any order: a row's noise goes with its id
    rows = [o[::-1] for o in obs]
    got = ro.actor_eval(dict(zip(ro._names, rows)) if len(rows) > 1 else rows[0], ids, step=12)
    wa, wl, wv, feat = harness_eval(lib, actor, rows, ids, 12, 2**40 + 5, deterministic)
    assert got[0].dtype == env._rollout().action_dtype
    assert same(got[0].reshape(wa.shape), wa.astype(got[0].dtype))
    assert same(got[1], wl) and same(got[2], wv)
    assert len(np.unique(feat)) >= 3, "the features must not sit on one clamp"
    if task == "Pendulum-v1" and not deterministic:
        assert (got[0] == -2.0).any() and (got[0] == 2.0).any() and ((got[0] > -2.0) & (got[0] < 2.0)).any()
    if not deterministic and actor.kind == 0:
        assert len(np.unique(got[0])) > 1
    ro.close()
    env.close()


def run_pair(lib, task, n=N, horizons=3, deterministic=False, device=None, **kw):
    """Pool A collects; its twin B is driven from the host through actor_eval + step.  Everything must be equal.
    `device`: A's (a list: a sharded pool, whose moments are sums of the shards' and so not compared)."""
    moments = device is None
    env_a, ro_a, actor = open_ro(task, n, deterministic=deterministic, moments=moments,
                                 **(dict(kw, device=device) if device else kw))
    env_b, ro_b, _ = open_ro(task, n, deterministic=deterministic, moments=moments, **kw)
    assert same(ro_a.reset(), ro_b.reset())
    out = []
    for h in range(horizons):
        ro_a.collect()
        logp, value = [], []
        for t in range(T):
            obs = obs_list(ro_b, ro_b.batch().obs, t)
            a, lp, v = ro_b.actor_eval(dict(zip(ro_b._names, obs)) if len(obs) > 1 else obs[0])
            if h == 0 and t == 1:  # the loop's evaluator is the g++ build's
                wa, wl, wv, _ = harness_eval(lib, actor, obs, env_b.all_env_ids, ro_b.counters["steps"], 9, deterministic)
                assert same(a.reshape(wa.shape), wa.astype(a.dtype)) and same(lp, wl) and same(v, wv)
                if device is not None:  # the sharded pool's direct form: every row by the shard that holds its env
                    ids = env_b.all_env_ids[::-1].copy()
                    rows = [o[::-1] for o in obs]
                    arg = dict(zip(ro_b._names, rows)) if len(rows) > 1 else rows[0]
                    assert same(ro_a.actor_eval(arg, ids, step=5), ro_b.actor_eval(arg, ids, step=5))
                    assert env_a._rollout().actor_shape() == env_b._rollout().actor_shape()
            ro_b.step(a)
            logp.append(lp)
            value.append(v)
        obs = obs_list(ro_b, ro_b.batch().obs, T)
        value.append(ro_b.actor_eval(dict(zip(ro_b._names, obs)) if len(obs) > 1 else obs[0])[2])
        ba, bb = ro_a.batch(), ro_b.batch()
        for name in ("obs", "action", "reward", "term", "trunc", "mask"):
            assert same(getattr(ba, name), getattr(bb, name)), (task, h, name)
        assert same(ba.logp, np.stack(logp)) and same(ba.value, np.stack(value)), (task, h)
        assert ro_a.counters == ro_b.counters
        if moments and any(np.dtype(d).kind == "f" for k, d, _ in env_b._rollout().state_keys if k in ro_b._names):
            assert same(ro_a.moments(), ro_b.moments())
        adv, ret = ro_a.gae(gamma=0.99, lam=0.95)          # the stored values ...
        assert same((adv, ret), ro_a.gae(ba.value, 0.99, 0.95))  # ... are the same call with the same array
        assert same((adv, ret), ro_b.gae(np.stack(value), 0.99, 0.95))
        if h != 1:
            assert same(tuple(ro_a.episodes()), tuple(ro_b.episodes()))
        out.append(ba)
        ro_a.next()
        ro_b.next()
    for x in (ro_a, ro_b):
        x.close()
    for x in (env_a, env_b):
        x.close()
    return out


@pytest.mark.parametrize("task", list(TASKS))
def test_collect_equals_the_host_driven_loop(lib, task):
    out = run_pair(lib, task)
    if task == "CartPole-v1":  # every env truncates in step 2 and 6: masked rows inside and at the start of a horizon
        assert out[0].trunc[2].all() and not out[0].mask[3].any() and not out[1].mask[0].any()
        assert np.isfinite(out[0].logp).all() and len(np.unique(out[0].action)) == 2


def test_deterministic_collect(lib):
    out = run_pair(lib, "CartPole-v1", horizons=1, deterministic=True)
    again = run_pair(lib, "CartPole-v1", horizons=1, deterministic=True)
    assert same(out[0].action, again[0].action)
    run_pair(lib, "HalfCheetah-v4", horizons=1, deterministic=True)


@pytest.mark.parametrize("n", [1, 1025])
def test_one_env_and_many(lib, n):
    run_pair(lib, "CartPole-v1", n=n, horizons=1)


def test_env_id_offset(lib):
    a = run_pair(lib, "CartPole-v1", n=65, horizons=1, env_id_offset=3)
    b = run_pair(lib, "CartPole-v1", n=65, horizons=1)
    assert not same(a[0].action, b[0].action)   # the noise is keyed by the global id


def test_sharded_pool_equals_the_unsharded_pool(lib):
    run_pair(lib, "CartPole-v1", n=130, horizons=2, device=[0, 0])
    run_pair(lib, "Pendulum-v1", n=130, horizons=1, device=[0, 0])


def test_split_collect_equals_one_collect():
    env_a, ro_a, _ = open_ro("HalfCheetah-v4", N)
    env_b, ro_b, _ = open_ro("HalfCheetah-v4", N)
    ro_a.reset()
    ro_b.reset()
    ro_a.collect(3)
    assert ro_a.t == 3
    ro_a.collect(4)
    ro_b.collect(7)
    ba, bb = ro_a.batch(), ro_b.batch()
    assert same(tuple(ba), tuple(bb)) and ba.value.shape == (T + 1, N) and ba.logp.shape == (T, N)
    assert same(ro_a.moments(), ro_b.moments()) and ro_a.counters == ro_b.counters
    for x in (ro_a, ro_b, env_a, env_b):
        x.close()


def test_torch_device_forms_equal_the_numpy_forms():
    torch = pytest.importorskip("torch")
    from envpool_amd import torch_interop as ti

    env_a, ro_a, actor = open_ro("HalfCheetah-v4", N)
    env_b, ro_b, _ = open_ro("HalfCheetah-v4", N)
    pool = env_b._rollout()
    dev = torch.device("cuda", pool.device)
    ro_a.reset()
    ro_b.reset()
    ro_a.collect(3)
    ti.rollout_collect_device(pool, 3)
    ro_a.collect()
    ti.rollout_collect_device(pool)
    ba = ro_a.batch()
    view = ti.rollout_view_device(pool)
    logp, value = ti.actor_view_device(pool)
    assert same(ba.obs, view["obs"].cpu().numpy()) and same(ba.action, view["action"].cpu().numpy())
    assert same(ba.logp, logp.cpu().numpy()) and same(ba.value, value.cpu().numpy())
    ids = torch.arange(N, dtype=torch.int32, device=dev)
    got = ti.actor_eval_device(pool, view["obs"][2].contiguous(), ids, 5)
    want = ro_a.actor_eval(ba.obs[2], np.arange(N, dtype=np.int32), 5)
    assert same(tuple(x.cpu().numpy() for x in got), want)
    for x in (ro_a, ro_b, env_a, env_b):
        x.close()


def test_refusals():
    env = make("CartPole-v1", 8)
    actor = Actor.random(env, hidden=32, blocks=1)
    with pytest.raises(ValueError, match="no rollout collector"):     # attach without a collector
        env._rollout().actor_begin(actor)
    ro = env.rollout(horizon=2, episodes=4)
    with pytest.raises(ValueError, match="no actor"):
        ro.collect()
    pend = envpool.make_spec("Pendulum-v1")
    for wrong in (Actor.random(pend, hidden=32),                                              # F, H and kind
                  Actor.random(dict(features=4, kind=0, actions=3, low=[], high=[], obs_low=np.zeros(4),
                                    obs_high=np.ones(4)), hidden=32),                         # H
                  Actor.random(dict(features=5, kind=0, actions=2, low=[], high=[], obs_low=np.zeros(5),
                                    obs_high=np.ones(5)), hidden=32),                         # F
                  Actor.random(dict(features=4, kind=1, actions=2, low=[-1, -1], high=[1, 1], obs_low=np.zeros(4),
                                    obs_high=np.ones(4)), hidden=32)):                        # kind
        with pytest.raises(ValueError, match="an actor of F"):
            ro.attach(wrong)
        with pytest.raises(ValueError, match="an actor of F"):   # the engine's own check, behind the Python one
            env._rollout().actor_begin(wrong, actions=2)
    ro.attach(actor)
    assert env._rollout().actor_shape() == (4, 2, 0, 0)   # F, H, kind, flags
    ro.attach(actor, deterministic=True)                   # a new actor replaces the one before
    assert env._rollout().actor_shape() == (4, 2, 0, 1)
    with pytest.raises(ValueError, match="not been reset"):
        ro.collect()
    ro.reset()
    with pytest.raises(ValueError, match="pass the horizon"):
        ro.collect(3)
    ro.collect()
    with pytest.raises(ValueError, match="horizon of 2 steps is full"):
        ro.collect()
    with pytest.raises(ValueError, match="steps"):
        ro.collect(0)
    ro.close()
    env.close()
    env = envpool.make("TicTacToe-v1", "gymnasium", num_envs=4)
    with pytest.raises(RuntimeError, match="rollout not implemented for this environment"):
        env._rollout()
    with pytest.raises(RuntimeError, match="rollout not implemented for this environment"):
        env.device_pool.actor_begin(actor)
    env.close()
    from atari_util import plugin_path, register_synthetic_ids

    register_synthetic_ids()
    env = envpool.make("SynthFire-v5", env_type="gymnasium", num_envs=4, seed=1, emulator_lib=plugin_path(),
                       base_path="/synthetic")
    with pytest.raises(RuntimeError, match="rollout not implemented for this environment"):
        env.rollout(horizon=2).attach(actor)
    env.close()
