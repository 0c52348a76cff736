"""Non-default task options of the gym-MuJoCo families: every kernel variant that serves a family against
the fp64 oracle (oracle/mjcpu), which tests/test_ref_mujoco.py::test_task_options_are_the_reference_config
pins bit for bit to the reference's own wrappers under the same options.  The option sets are
MJ_OPTION_CASES (tests/mj_util.py): frame_skip 1 and odd values, exclude_current_positions_from_observation
off, terminate_when_unhealthy off under both healthy-reward rules, tight healthy ranges, the contact-force /
contact-cost / observation clamps, reset scales, the Pusher's cylinder box, zero and large reset noise.

Per case and kernel variant: obs shape, reset rows (info and reward bit for bit, -0.0 included), a
teacher-forced rollout through auto-resets (obs rtol 1e-9 / atol 1e-10, bookkeeping exact), and a short
free-running horizon.  Plus: explicit defaults == omitted options, and `ant_sub` never changes results."""
import numpy as np
import pytest

from envpool_amd.core.device_pool import DevicePool
from oracle.orc import Oracle
from tests.mj_util import MJ_OPTION_CASES, option_case

pytestmark = pytest.mark.gpu

_PLANAR = [{"planar_layout": 1}, {"planar_layout": 2}, {"planar_layout": 4, "planar_waves": 1},
           {"planar_layout": 4, "planar_waves": 2}]
# every kernel variant that serves a family (the engine keys that select them)
KERNEL_VARIANTS = {
    "HalfCheetah": _PLANAR, "Walker2d": _PLANAR,
    "Hopper": [{"planar_layout": 0}, {"planar_layout": 1}],
    "Humanoid": [{"hum_sort": 0}, {"hum_sort": 1}], "HumanoidStandup": [{"hum_sort": 0}, {"hum_sort": 1}],
}
_AMAX = {"InvertedPendulum": 3.0, "Pusher": 2.0, "Humanoid": 0.4, "HumanoidStandup": 0.4}
_BOOK = ("done", "trunc", "elapsed_step", "step_type", "discount", "info:env_id")


def _cases():
    out = []
    for case in sorted(MJ_OPTION_CASES):
        family = option_case(case)[3]
        for v in KERNEL_VARIANTS.get(family, [{}]):
            tag = "-".join(f"{k}{x}" for k, x in v.items()) or "default"
            out.append(pytest.param(case, v, id=f"{case}-{tag}"))
    return out


def _info_keys(d):
    return [k for k in d if k.startswith("info:") and k not in ("info:env_id", "info:players.env_id")]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


@pytest.mark.parametrize("case,variant", _cases())
def test_kernel_options_match_oracle(case, variant):
    task, max_steps, extra, family, params, S, expect = option_case(case)
    humanoid = family.startswith("Humanoid")
    n, steps, seed = (32, 30, 7) if humanoid else (96, 45, 7)
    pool = DevicePool(family, n, seed=seed, max_episode_steps=max_steps,
                      params={**params, **variant})
    orc = Oracle(task, n, seed=seed, max_episode_steps=max_steps, extra=extra)
    ids = np.arange(n, dtype=np.int32)
    nobs = dict((k, e) for k, _, e in orc.keys)["obs"]
    adim, amax = orc.action_elems, _AMAX.get(family, 1.0)
    cf_cols = 0
    if family == "Ant" and params.get("use_contact_force"):
        cf_cols = 6 * (14 - int(params.get("exclude_worldbody_contact_forces", 0)))

    def check_obs(a_obs, ring, tag):
        want = ring if S > 1 else ring[:, 0]
        assert a_obs.shape == want.shape, (tag, a_obs.shape, want.shape)
        if humanoid:  # PGS is not run to convergence: every row to 1e-5, the bulk to 1e-9 (test_gpu_mujoco.py)
            rel = (np.abs(a_obs - want) / (1.0 + np.abs(want))).reshape(n, -1).max(axis=1)
            assert rel.max() < 1e-5, (tag, rel.max())
            return rel
        a2, w2 = a_obs.reshape(n, S, nobs), want.reshape(n, S, nobs)
        k = nobs - cf_cols
        np.testing.assert_allclose(a2[..., :k], w2[..., :k], rtol=1e-9, atol=1e-10, err_msg=tag)
        if cf_cols:  # cfrc_ext (test_gpu_mujoco.py::test_ant_contact_force_observation)
            np.testing.assert_allclose(a2[..., k:], w2[..., k:], rtol=1e-8, atol=1e-9, err_msg=tag)
        return np.zeros(n)

    def check_step(a, b, ring, tag):
        rel = check_obs(a["obs"], ring, tag)
        tol = dict(rtol=1e-5, atol=1e-5) if humanoid else dict(rtol=1e-9, atol=2e-9)
        np.testing.assert_allclose(a["reward"].ravel(), b["reward"].ravel(),
                                   **(dict(rtol=1e-5, atol=1e-4) if humanoid else dict(rtol=1e-6, atol=1e-6)),
                                   err_msg=f"reward {tag}")
        for k in _info_keys(b):
            t = dict(rtol=1e-8, atol=2e-9) if k == "info:reward_contact" else tol
            np.testing.assert_allclose(a[k].ravel(), b[k].ravel(), **t, err_msg=f"{k} {tag}")
        for k in _BOOK:
            np.testing.assert_array_equal(a[k].ravel(), b[k].ravel(), err_msg=f"{k} {tag}")
        # reset rows are constants and uniform draws: info and reward bit for bit, the sign of zero included
        rows = b["elapsed_step"].ravel() == 0
        for k in _info_keys(b) + ["reward"]:
            assert np.array_equal(_bits(a[k].ravel()[rows]), _bits(b[k].ravel()[rows])), (k, tag)
        return rel

    def push(ring, b):
        first = b["elapsed_step"].ravel() == 0
        ring = np.concatenate([ring[:, 1:], b["obs"][:, None, :]], axis=1)
        ring[first] = b["obs"][first][:, None, :]
        return ring

    pool.reset(ids)
    a, b = pool.recv_dict(), orc.reset()
    assert list(a.keys()) == list(b.keys())
    assert b["obs"].shape == (n, nobs)
    assert a["obs"].shape == ((n, S, nobs) if S > 1 else (n, nobs))
    ring = np.repeat(b["obs"][:, None, :], S, axis=1)
    np.testing.assert_allclose(a["obs"], ring if S > 1 else ring[:, 0], rtol=1e-11, atol=1e-12)
    check_step(a, b, ring, "reset")

    # teacher forced: the oracle's state every step, through terminations / truncations and auto-resets
    rng = np.random.default_rng(3)
    rels, terms, resets = [], 0, 0
    for t in range(steps):
        pool.set_state(orc.get_state())
        act = rng.uniform(-1.2 * amax, 1.2 * amax, size=(n, adim))
        pool.send(ids, act)
        a, b = pool.recv_dict(), orc.step(act)
        ring = push(ring, b)
        rels.append(check_step(a, b, ring, f"{case} step {t}"))
        terms += int((b["done"] & ~b["trunc"]).sum())
        resets += int((b["elapsed_step"] == 0).sum())
    assert resets > 0, case  # at least one auto-reset row was compared
    if expect == "term":
        assert terms > 0, case
    else:
        assert terms == 0, case
    if humanoid:
        assert (np.concatenate(rels) < 1e-9).mean() > 0.99

    # free running from a fresh reset: per env, agreement until rounding differences have grown past 1e-5
    pool.reset(ids)
    a, b = pool.recv_dict(), orc.reset()
    ring = np.repeat(b["obs"][:, None, :], S, axis=1)
    live = np.ones(n, bool)
    for t in range(12):
        act = rng.uniform(-amax, amax, size=(n, adim))
        pool.send(ids, act)
        a, b = pool.recv_dict(), orc.step(act)
        ring = push(ring, b)
        want = (ring if S > 1 else ring[:, 0]).reshape(n, -1)
        rel = (np.abs(a["obs"].reshape(n, -1) - want) / (1e-2 + np.abs(want))).max(axis=1)
        live &= rel <= 1e-5
        for k in ("done", "trunc", "elapsed_step", "step_type"):
            np.testing.assert_array_equal(a[k].ravel()[live], b[k].ravel()[live], err_msg=f"{k} free {t}")
    assert live.mean() >= 0.5, (case, live.mean())


def test_reacher_refuses_goals_beyond_the_target_range():
    """The kernel holds the target's slides at their reset values, which is exact only while no goal can
    leave their range (-0.27, 0.27): a larger reset_goal_scale is refused, not computed wrongly."""
    with pytest.raises(ValueError, match="reset_goal_scale"):
        DevicePool("Reacher", 8, seed=0, max_episode_steps=10, params={"reset_goal_scale": 0.3})


# ---- explicit defaults: every option at its default value gives the bytes of the omitted option ------
_DEFAULTS = {
    "HalfCheetah": dict(frame_skip=5, frame_stack=1, exclude_current_positions_from_observation=1,
                        ctrl_cost_weight=0.1, forward_reward_weight=1.0, reset_noise_scale=0.1),
    "Ant": dict(frame_skip=5, frame_stack=1, exclude_current_positions_from_observation=1,
                terminate_when_unhealthy=1, legacy_healthy_reward=1, ctrl_cost_weight=0.5,
                forward_reward_weight=1.0, healthy_reward=1.0, healthy_z_min=0.2, healthy_z_max=1.0,
                reset_noise_scale=0.1, use_contact_force=0, exclude_worldbody_contact_forces=0,
                contact_cost_weight=5e-4, contact_force_min=-1.0, contact_force_max=1.0),
    "Walker2d": dict(frame_skip=4, frame_stack=1, exclude_current_positions_from_observation=1,
                     terminate_when_unhealthy=1, legacy_healthy_reward=1, ctrl_cost_weight=1e-3,
                     forward_reward_weight=1.0, healthy_reward=1.0, healthy_z_min=0.8, healthy_z_max=2.0,
                     healthy_angle_min=-1.0, healthy_angle_max=1.0, velocity_min=-10.0, velocity_max=10.0,
                     reset_noise_scale=5e-3),
    "Hopper": dict(frame_skip=4, frame_stack=1, exclude_current_positions_from_observation=1,
                   terminate_when_unhealthy=1, legacy_healthy_reward=1, ctrl_cost_weight=1e-3,
                   forward_reward_weight=1.0, healthy_reward=1.0, velocity_min=-10.0, velocity_max=10.0,
                   healthy_state_min=-100.0, healthy_state_max=100.0, healthy_angle_min=-0.2,
                   healthy_angle_max=0.2, healthy_z_min=0.7, reset_noise_scale=5e-3),
    "Swimmer": dict(frame_skip=4, frame_stack=1, exclude_current_positions_from_observation=1,
                    forward_reward_weight=1.0, ctrl_cost_weight=1e-4, reset_noise_scale=0.1),
    "Reacher": dict(frame_skip=2, frame_stack=1, ctrl_cost_weight=1.0, reward_after_step=0,
                    obs_include_z_distance=1, dist_cost_weight=1.0, reset_qpos_scale=0.1,
                    reset_qvel_scale=0.005, reset_goal_scale=0.2),
    "Pusher": dict(frame_skip=5, frame_stack=1, ctrl_cost_weight=0.1, dist_cost_weight=1.0,
                   near_cost_weight=0.5, reward_after_step=0, weighted_reward_info=0, reset_qvel_scale=0.005,
                   cylinder_x_min=-0.3, cylinder_x_max=0.0, cylinder_y_min=-0.2, cylinder_y_max=0.2,
                   cylinder_dist_min=0.17),
    "InvertedPendulum": dict(frame_skip=2, frame_stack=1, healthy_reward=1.0, reward_if_not_terminated=0,
                             healthy_z_min=-0.2, healthy_z_max=0.2, reset_noise_scale=0.01),
    "InvertedDoublePendulum": dict(frame_skip=5, frame_stack=1, healthy_reward=10.0,
                                   reward_if_not_terminated=0, constraint_obs_dim=3, healthy_z_max=1.0,
                                   observation_min=-10.0, observation_max=10.0, reset_noise_scale=0.1),
    "Humanoid": dict(frame_skip=5, frame_stack=1, exclude_current_positions_from_observation=1,
                     exclude_worldbody_observations=0, exclude_root_actuator_forces=0,
                     forward_reward_weight=1.25, ctrl_cost_weight=0.1, healthy_reward=5.0,
                     contact_cost_weight=5e-7, contact_cost_max=10.0, reset_noise_scale=1e-2,
                     legacy_healthy_reward=1, use_contact_force=0, terminate_when_unhealthy=1,
                     healthy_z_min=1.0, healthy_z_max=2.0),
    "HumanoidStandup": dict(frame_skip=5, frame_stack=1, exclude_current_positions_from_observation=1,
                            exclude_worldbody_observations=0, exclude_root_actuator_forces=0,
                            forward_reward_weight=1.0, ctrl_cost_weight=0.1, healthy_reward=1.0,
                            contact_cost_weight=5e-7, contact_cost_max=10.0, reset_noise_scale=1e-2),
}


@pytest.mark.parametrize("family", sorted(_DEFAULTS))
def test_explicit_defaults_are_the_omitted_defaults(family):
    """The task options of the reference's DefaultConfig() (envpool_amd/mujoco/gym native_params), each
    passed at its default value, give the same bytes as a pool that is given none of them."""
    n = 64
    orc = Oracle(family, 1, seed=0, max_episode_steps=10)
    adim, amax = orc.action_elems, _AMAX.get(family, 1.0)
    acts = np.random.default_rng(1).uniform(-amax, amax, size=(6, n, adim))
    ids = np.arange(n, dtype=np.int32)
    outs = []
    for params in ({}, _DEFAULTS[family]):
        p = DevicePool(family, n, seed=4, max_episode_steps=4, params=params)
        p.reset(ids)
        seq = [p.recv_dict()]
        for t in range(6):
            p.send(ids, acts[t])
            seq.append(p.recv_dict())
        outs.append((seq, p.get_state()))
    (sa, ga), (sb, gb) = outs
    for t, (a, b) in enumerate(zip(sa, sb)):
        assert list(a.keys()) == list(b.keys())
        for k in a:
            assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (family, t, k)
    assert ga.tobytes() == gb.tobytes()


# ---- ant_sub: mj_steps per unit of the Ant step kernel's work queue: never changes results -------------
@pytest.mark.parametrize("use_contact_force", [0, 1])
@pytest.mark.parametrize("frame_skip", [1, 3, 5, 7])
def test_ant_sub_never_changes_results(frame_skip, use_contact_force):
    """Every ant_sub in 1..frame_skip, including those that do not divide it (the last unit of an env-step is
    then shorter), bit-identical to ant_sub = 1 on every state key and the device state.  4096 envs: 256
    chunks of 16 envs queued at once; one partial env_id send and one reset of a subset on the way."""
    n = 4096
    rng = np.random.default_rng(frame_skip)
    acts = rng.uniform(-1, 1, size=(8, n, 8))
    ids = np.arange(n, dtype=np.int32)
    part = np.sort(rng.choice(n, size=1500, replace=False)).astype(np.int32)
    params = {"frame_skip": frame_skip, "use_contact_force": use_contact_force,
              "post_constraint": use_contact_force}
    ref = None
    for sub in range(1, frame_skip + 1):
        p = DevicePool("Ant", n, seed=2, max_episode_steps=1000, params={**params, "ant_sub": sub})
        p.reset(ids)
        seq = [p.recv_dict()]
        for t in range(8):
            if t == 3:
                p.send(part, acts[t][part])
            elif t == 5:
                p.reset(part)
            else:
                p.send(ids, acts[t])
            seq.append(p.recv_dict())
        run = (seq, p.get_state())
        p.close()
        if ref is None:
            ref = run
            continue
        for t, (a, b) in enumerate(zip(ref[0], run[0])):
            for k in a:
                assert a[k].tobytes() == b[k].tobytes(), (frame_skip, use_contact_force, sub, t, k)
        assert ref[1].tobytes() == run[1].tobytes(), (frame_skip, use_contact_force, sub)
