"""Raw access to oracle/mjcpu for invariant tests (test infrastructure)."""
import ctypes

import numpy as np

from oracle.orc import Oracle


class _H(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("h", ctypes.c_void_p), ("n", ctypes.c_int)]


class RawMj:
    """extra = [frame_skip, ctrl_w, fwd_w, noise, no_contact, no_limit, no_act,
    no_passive]"""

    def __init__(self, task, extra=()):
        self.o = Oracle(task, 1, seed=0, max_episode_steps=1000, extra=extra)
        self.L = self.o.lib
        self.inner = ctypes.cast(self.o.h, ctypes.POINTER(_H)).contents.h
        sc = np.zeros(256)
        self.L.mjcpu_model_scalars.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self.L.mjcpu_model_scalars(self.inner, sc.ctypes.data)
        self.nq, self.nv, self.nu, self.nbody, self.ngeom = (int(x) for x in sc[:5])
        self.meaninertia, self.total_mass = sc[5], sc[6]
        k = 7
        self.body_mass = sc[k:k + self.nbody].copy(); k += self.nbody
        self.dof_invweight0 = sc[k:k + self.nv].copy(); k += self.nv
        self.body_invweight0 = sc[k:k + 2 * self.nbody].reshape(-1, 2).copy()
        vp = ctypes.c_void_p
        self.L.mjcpu_raw_set.argtypes = [vp, ctypes.c_int, vp, vp, vp]
        self.L.mjcpu_raw_step.argtypes = [vp, ctypes.c_int, ctypes.c_int]
        self.L.mjcpu_raw_get.argtypes = [vp, ctypes.c_int, vp, vp, vp]

    def set(self, qpos, qvel, ctrl=None):
        qpos = np.ascontiguousarray(qpos, dtype=np.float64)
        qvel = np.ascontiguousarray(qvel, dtype=np.float64)
        ctrl = np.zeros(self.nu) if ctrl is None else np.ascontiguousarray(ctrl, dtype=np.float64)
        self.L.mjcpu_raw_set(self.inner, 0, qpos.ctypes.data, qvel.ctypes.data, ctrl.ctypes.data)

    def set_warm(self, qpos, qvel, ctrl, warm):
        """State of a running simulation incl. qacc_warmstart, no forward pass."""
        arrs = [np.ascontiguousarray(x, dtype=np.float64) for x in (qpos, qvel, ctrl, warm)]
        self.L.mjcpu_raw_set_warm.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4
        self.L.mjcpu_raw_set_warm(self.inner, 0, *[a.ctypes.data for a in arrs])

    def observed(self):
        """cinert, cvel, qfrc_actuator, cfrc_ext of the last forward evaluation."""
        nb, nv = self.nbody, self.nv
        out = np.zeros(nb * 22 + nv)
        self.L.mjcpu_raw_observed.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        self.L.mjcpu_raw_observed(self.inner, 0, out.ctypes.data)
        return (out[:nb * 10].reshape(nb, 10), out[nb * 10:nb * 16].reshape(nb, 6),
                out[nb * 16:nb * 16 + nv], out[nb * 16 + nv:].reshape(nb, 6))

    def step(self, n=1):
        self.L.mjcpu_raw_step(self.inner, 0, n)

    def get(self):
        qpos, qvel, misc = np.zeros(self.nq), np.zeros(self.nv), np.zeros(16)
        self.L.mjcpu_raw_get(self.inner, 0, qpos.ctypes.data, qvel.ctypes.data, misc.ctypes.data)
        names = ["ke", "pe", "ncon", "nefc", "iters", "time", "fmin", "resid",
                 "asym", "torso_z", "fsum"]
        return qpos, qvel, dict(zip(names, misc))


# ---- positional `extra` of mjcpu_create / ref_mujoco_driver.cc (oracle/mjcpu/tasks.c) --------
_EXTRA_NAMES = {
    "frame_skip": 0, "ctrl_cost_weight": 1, "forward_reward_weight": 2, "reset_noise_scale": 3,
    "disable_contact": 4, "disable_limit": 5, "disable_actuation": 6, "disable_passive": 7,
    "integrator": 8, "timestep": 9, "reward_if_not_terminated": 10, "constraint_obs_dim": 11,
    "use_contact_force": 12, "post_constraint": 13, "exclude_worldbody": 14,
    "legacy_healthy_reward": 15, "reward_after_step": 16, "obs_include_z": 17,
    "disable_selfcollide": 18, "exclude_root_actuator": 19, "dist_cost_weight": 20,
    "near_cost_weight": 21, "weighted_reward_info": 22, "frame_stack": 23, "warmstart_rule": 24,
    # task options of the reference's DefaultConfig(); NaN = the family's default
    "exclude_current_positions_from_observation": 25, "terminate_when_unhealthy": 26,
    "healthy_reward": 27, "healthy_z_min": 28, "healthy_z_max": 29, "healthy_angle_min": 30,
    "healthy_angle_max": 31, "velocity_min": 32, "velocity_max": 33, "healthy_state_min": 34,
    "healthy_state_max": 35, "contact_cost_weight": 36, "contact_cost_max": 37,
    "contact_force_min": 38, "contact_force_max": 39, "observation_min": 40, "observation_max": 41,
    "reset_qpos_scale": 42, "reset_qvel_scale": 43, "reset_goal_scale": 44, "cylinder_x_min": 45,
    "cylinder_x_max": 46, "cylinder_y_min": 47, "cylinder_y_max": 48, "cylinder_dist_min": 49,
}
_OPTION_BASE = 25


def mj_extra(task, **over):
    """Full `extra` tuple for `task` with the task's own defaults and `over` applied."""
    base = task.replace("V5", "")
    fs = 4 if base in ("Walker2d", "Swimmer", "Hopper") else 2 if base in ("InvertedPendulum", "Reacher") else 5
    cw = {"Ant": 0.5, "Walker2d": 1e-3, "Hopper": 1e-3, "Reacher": 1.0, "Swimmer": 1e-4}.get(base, 0.1)
    fw = 1.25 if base == "Humanoid" else 1.0
    noise = 5e-3 if base in ("Walker2d", "Hopper") else 1e-2 if base in ("InvertedPendulum", "Humanoid", "HumanoidStandup") else 0.1
    ex = [fs, cw, fw, noise, 0, 0, 0, 0, -1, 0, 0, 3, 0, 0, 0, -1, 0, 1, 0, 0, 1.0, 0.5, 0, 1, 0]
    ex += [float("nan")] * (len(_EXTRA_NAMES) - _OPTION_BASE)
    for k, v in over.items():
        ex[_EXTRA_NAMES[k]] = float(v)
    return tuple(float(v) for v in ex)


# registered gym-MuJoCo ids -> (oracle task, max_episode_steps, options); the options are those
# envpool/mujoco/gym/registration.py:38-93 passes for the version
GYM_VARIANTS = {
    "HalfCheetah-v4": ("HalfCheetah", 1000, {}),
    "HalfCheetah-v5": ("HalfCheetah", 1000, dict(post_constraint=1)),
    "Ant-v3": ("Ant", 1000, dict(use_contact_force=1)),
    "Ant-v4": ("Ant", 1000, {}),
    "Ant-v5": ("Ant", 1000, dict(use_contact_force=1, post_constraint=1, exclude_worldbody=1,
                                 legacy_healthy_reward=0)),
    "Walker2d-v4": ("Walker2d", 1000, {}),
    "Walker2d-v5": ("Walker2dV5", 1000, dict(post_constraint=1, legacy_healthy_reward=0)),
    "Hopper-v4": ("Hopper", 1000, {}),
    "Hopper-v5": ("Hopper", 1000, dict(post_constraint=1, legacy_healthy_reward=0)),
    "Swimmer-v4": ("Swimmer", 1000, {}),
    "Swimmer-v5": ("Swimmer", 1000, dict(post_constraint=1)),
    "Reacher-v4": ("Reacher", 50, {}),
    "Reacher-v5": ("Reacher", 50, dict(post_constraint=1, reward_after_step=1, obs_include_z=0)),
    "Pusher-v4": ("Pusher", 100, {}),
    "Pusher-v5": ("PusherV5", 100, dict(post_constraint=1, reward_after_step=1,
                                        weighted_reward_info=1)),
    "InvertedPendulum-v4": ("InvertedPendulum", 1000, {}),
    "InvertedPendulum-v5": ("InvertedPendulum", 1000, dict(post_constraint=1,
                                                           reward_if_not_terminated=1)),
    "InvertedDoublePendulum-v4": ("InvertedDoublePendulum", 1000, {}),
    "InvertedDoublePendulum-v5": ("InvertedDoublePendulum", 1000,
                                  dict(post_constraint=1, reward_if_not_terminated=1,
                                       constraint_obs_dim=1)),
    "Humanoid-v3": ("Humanoid", 1000, dict(use_contact_force=1)),
    "Humanoid-v4": ("Humanoid", 1000, {}),
    "Humanoid-v5": ("Humanoid", 1000, dict(use_contact_force=1, post_constraint=1,
                                           exclude_worldbody=1, exclude_root_actuator=1,
                                           legacy_healthy_reward=0)),
    "HumanoidStandup-v4": ("HumanoidStandup", 1000, {}),
    "HumanoidStandup-v5": ("HumanoidStandup", 1000, dict(post_constraint=1, exclude_worldbody=1,
                                                         exclude_root_actuator=1)),
}

_NATIVE_NAMES = {
    "use_contact_force": "use_contact_force", "post_constraint": "post_constraint",
    "legacy_healthy_reward": "legacy_healthy_reward", "reward_after_step": "reward_after_step",
    "obs_include_z": "obs_include_z_distance", "weighted_reward_info": "weighted_reward_info",
    "reward_if_not_terminated": "reward_if_not_terminated", "constraint_obs_dim": "constraint_obs_dim",
    "exclude_root_actuator": "exclude_root_actuator_forces",
    "frame_skip": "frame_skip", "ctrl_cost_weight": "ctrl_cost_weight",
    "forward_reward_weight": "forward_reward_weight", "reset_noise_scale": "reset_noise_scale",
    "dist_cost_weight": "dist_cost_weight", "near_cost_weight": "near_cost_weight",
    "frame_stack": "frame_stack",
}
_NATIVE_NAMES.update((k, k) for k, i in _EXTRA_NAMES.items() if i >= _OPTION_BASE)


def native_variant(name, **more):
    """(DevicePool family, params under the reference's config key names) of a GYM_VARIANTS id."""
    task, max_steps, over = GYM_VARIANTS[name]
    over = {**over, **more}
    family = task.replace("V5", "")
    params = {"post_constraint": 0}
    if task.endswith("V5"):
        params["xml_v5"] = 1
    for k, v in over.items():
        if k == "exclude_worldbody":
            params["exclude_worldbody_contact_forces" if family == "Ant"
                   else "exclude_worldbody_observations"] = v
        else:
            params[_NATIVE_NAMES[k]] = v
    if family in ("HalfCheetah", "Walker2d", "Hopper", "Ant"):
        params.setdefault("precision", 1)
    return family, max_steps, params


# ---- non-default task options: one table for the oracle-vs-reference pin (test_ref_mujoco.py) and the
# kernels-vs-oracle tests (test_gpu_mujoco_options.py).  case id -> (registered id it starts from,
# max_episode_steps, options, expectation).  Every key of the MuJoCo families' native_params except
# precision, xml_v5 and the engine keys takes a non-default value in at least one case.  Expectation:
#   "term"   unhealthy terminations (done without trunc) and auto-resets happen within the run
#   "noterm" terminate_when_unhealthy=False: no terminations, the short episodes truncate instead
#   "trunc"  no health rule: the short episodes truncate and auto-reset
# `frame_stack` has no oracle position of its own (the port returns single frames): the GPU test stacks
# the oracle's frames itself, the reference pin leaves it out (test_frame_stack_is_the_reference_ring).
_NOTERM = dict(terminate_when_unhealthy=0)
MJ_OPTION_CASES = {
    "HalfCheetah-fs1-pos": ("HalfCheetah-v4", 30, dict(
        frame_skip=1, exclude_current_positions_from_observation=0, ctrl_cost_weight=0.0,
        forward_reward_weight=-0.5), "trunc"),
    "HalfCheetah-fs3-noise": ("HalfCheetah-v4", 30, dict(
        frame_skip=3, reset_noise_scale=0.5, frame_stack=2), "trunc"),
    "HalfCheetah-fs7-still": ("HalfCheetah-v5", 30, dict(
        frame_skip=7, reset_noise_scale=0.0, exclude_current_positions_from_observation=0), "trunc"),
    "Walker2d-fs1-pos-tight": ("Walker2d-v4", 1000, dict(
        frame_skip=1, exclude_current_positions_from_observation=0, healthy_z_min=1.1,
        healthy_z_max=1.4, healthy_angle_min=-0.15, healthy_angle_max=0.15, velocity_min=-0.5,
        velocity_max=0.75), "term"),
    "Walker2d-noterm-legacy": ("Walker2d-v4", 30, dict(
        _NOTERM, legacy_healthy_reward=1, healthy_reward=2.5, healthy_z_min=1.15, ctrl_cost_weight=0.0,
        frame_skip=3), "noterm"),
    "Walker2d-noterm-v5": ("Walker2d-v5", 30, dict(
        _NOTERM, legacy_healthy_reward=0, healthy_reward=0.5, healthy_z_min=1.15,
        forward_reward_weight=-1.0, reset_noise_scale=0.0), "noterm"),
    "Walker2d-fs5-noise": ("Walker2d-v4", 1000, dict(
        frame_skip=5, reset_noise_scale=0.5, healthy_angle_min=-0.5, healthy_angle_max=0.5), "term"),
    "Hopper-fs1-pos": ("Hopper-v4", 1000, dict(
        frame_skip=1, exclude_current_positions_from_observation=0, healthy_z_min=1.22,
        velocity_min=-0.5, velocity_max=0.5), "term"),
    "Hopper-state-range": ("Hopper-v5", 1000, dict(
        frame_skip=5, healthy_state_min=-1.5, healthy_state_max=1.5, healthy_angle_min=-0.5,
        healthy_angle_max=0.5, healthy_z_min=0.5, healthy_reward=0.25), "term"),
    "Hopper-noterm-legacy": ("Hopper-v4", 30, dict(
        _NOTERM, legacy_healthy_reward=1, healthy_z_min=1.22, ctrl_cost_weight=0.0,
        reset_noise_scale=0.5), "noterm"),
    "Hopper-noterm-v5": ("Hopper-v5", 30, dict(
        _NOTERM, legacy_healthy_reward=0, healthy_angle_min=-0.05, healthy_angle_max=0.05,
        forward_reward_weight=-2.0, frame_skip=3), "noterm"),
    "Swimmer-fs1-pos": ("Swimmer-v4", 30, dict(
        frame_skip=1, exclude_current_positions_from_observation=0, forward_reward_weight=-2.0,
        ctrl_cost_weight=0.0), "trunc"),
    "Swimmer-fs7-noise": ("Swimmer-v5", 30, dict(frame_skip=7, reset_noise_scale=0.5), "trunc"),
    "Ant-fs1-pos": ("Ant-v4", 1000, dict(
        frame_skip=1, exclude_current_positions_from_observation=0, reset_noise_scale=0.0,
        healthy_z_min=0.6, frame_stack=2), "term"),
    "Ant-contact-clip": ("Ant-v5", 1000, dict(
        frame_skip=3, exclude_current_positions_from_observation=0, contact_force_min=-0.1,
        contact_force_max=0.1, contact_cost_weight=0.05, healthy_z_min=0.3, healthy_z_max=0.75,
        ctrl_cost_weight=0.0), "term"),
    "Ant-contact-v3": ("Ant-v3", 1000, dict(
        post_constraint=1, contact_force_min=-0.1, contact_force_max=0.1, frame_skip=7,
        reset_noise_scale=0.5, healthy_z_max=0.8), "term"),
    "Ant-noterm-legacy": ("Ant-v4", 30, dict(
        _NOTERM, legacy_healthy_reward=1, healthy_z_min=0.5, healthy_z_max=0.6, healthy_reward=3.0),
        "noterm"),
    "Ant-noterm-v5": ("Ant-v5", 30, dict(
        _NOTERM, legacy_healthy_reward=0, healthy_z_min=0.5, healthy_z_max=0.6,
        forward_reward_weight=-1.0), "noterm"),
    "Humanoid-pos-contact": ("Humanoid-v4", 1000, dict(
        frame_skip=3, exclude_current_positions_from_observation=0, use_contact_force=1,
        post_constraint=1, contact_cost_weight=1e-3, contact_cost_max=0.05, healthy_z_min=1.25),
        "term"),
    "Humanoid-noterm-legacy": ("Humanoid-v4", 12, dict(
        _NOTERM, legacy_healthy_reward=1, healthy_reward=2.0, healthy_z_min=1.3, healthy_z_max=1.45,
        ctrl_cost_weight=0.0, forward_reward_weight=-1.0, reset_noise_scale=0.1), "noterm"),
    "Humanoid-noterm-v5": ("Humanoid-v5", 12, dict(
        _NOTERM, healthy_z_min=1.395, healthy_z_max=1.45, frame_skip=1, reset_noise_scale=0.0),
        "noterm"),
    "HumanoidStandup-pos-contact": ("HumanoidStandup-v4", 12, dict(
        frame_skip=3, exclude_current_positions_from_observation=0, post_constraint=1,
        contact_cost_weight=1e-3, contact_cost_max=0.05, healthy_reward=0.5, forward_reward_weight=-1.0,
        ctrl_cost_weight=0.0, reset_noise_scale=0.1), "trunc"),
    "HumanoidStandup-fs1-still": ("HumanoidStandup-v5", 12, dict(
        frame_skip=1, reset_noise_scale=0.0), "trunc"),
    "Pusher-cylinder": ("Pusher-v4", 30, dict(
        frame_skip=3, reset_qvel_scale=0.5, cylinder_x_min=-0.5, cylinder_x_max=-0.2, cylinder_y_min=0.1,
        cylinder_y_max=0.4, cylinder_dist_min=0.3, ctrl_cost_weight=0.0), "trunc"),
    "Pusher-v5-fs1": ("Pusher-v5", 30, dict(
        frame_skip=1, reset_qvel_scale=0.0, cylinder_x_min=-0.1, cylinder_x_max=0.1,
        cylinder_y_min=-0.4, cylinder_y_max=-0.1, cylinder_dist_min=0.0), "trunc"),
    "Reacher-scales": ("Reacher-v4", 30, dict(
        frame_skip=1, reset_qpos_scale=0.5, reset_qvel_scale=0.5, reset_goal_scale=0.1,
        dist_cost_weight=2.0, ctrl_cost_weight=0.0), "trunc"),
    "Reacher-v5-still": ("Reacher-v5", 30, dict(
        frame_skip=5, reset_qpos_scale=0.0, reset_qvel_scale=0.0, reset_goal_scale=0.27), "trunc"),
    "InvertedPendulum-tight": ("InvertedPendulum-v4", 1000, dict(
        frame_skip=1, healthy_z_min=-0.05, healthy_z_max=0.1, reset_noise_scale=0.05, healthy_reward=2.0),
        "term"),
    "InvertedPendulum-v5-fs5": ("InvertedPendulum-v5", 1000, dict(frame_skip=5, reset_noise_scale=0.0),
                                "term"),
    "InvertedDoublePendulum-clip": ("InvertedDoublePendulum-v4", 1000, dict(
        observation_min=-0.5, observation_max=0.5, frame_skip=3, healthy_z_max=1.05, healthy_reward=3.0,
        frame_stack=2), "term"),
    "InvertedDoublePendulum-v5-fs1": ("InvertedDoublePendulum-v5", 1000, dict(
        frame_skip=1, reset_noise_scale=0.5, healthy_reward=5.0), "term"),
}


def option_case(case):
    """(oracle task, max_episode_steps, oracle `extra`, DevicePool family, DevicePool params, frame_stack,
    expectation) of an MJ_OPTION_CASES entry: one dict of options builds both sides."""
    gym_id, max_steps, opts, expect = MJ_OPTION_CASES[case]
    task, _, base = GYM_VARIANTS[gym_id]
    opts = dict(opts)
    stack = int(opts.pop("frame_stack", 1))
    family, _, params = native_variant(gym_id, **opts)
    if stack > 1:
        params["frame_stack"] = stack
    return task, max_steps, mj_extra(task, **{**base, **opts}), family, params, stack, expect
