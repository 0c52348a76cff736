"""oracle/mjcpu/tasks.c (the plain-C restatement of the gym task wrappers) against the
reference's OWN wrappers: envpool/mujoco/gym/*.h compiled in place inside the reference's own
AsyncEnvPool (oracle/_ref/libref_mujoco.so, oracle/ref_mujoco_driver.cc) over a mujoco.h shim
whose engine calls forward to oracle/mjcpu.  Same engine object code underneath both, so every
state key must agree BIT FOR BIT: this pins the reset draw order (libstdc++'s real
uniform_real_distribution / normal_distribution), rewards, healthy / termination rules,
observation and info assembly, post_constraint and the done / trunc / elapsed_step bookkeeping
of the restatement to reference code.  It does not pin the engine arithmetic.

Calling sequence as in the reference's own C++ test
(envpool/mujoco/gym/mujoco_gym_envpool_test.cc:27-56)."""
import ctypes
import json
import os

import numpy as np
import pytest

from oracle import orc
from oracle.orc import Oracle
from tests.mj_util import GYM_VARIANTS, MJ_OPTION_CASES, mj_extra, option_case

pytestmark = pytest.mark.skipif(not (orc.have_ref_mujoco() and orc.have_port()),
                                reason="oracle/_ref/libref_mujoco.so not built (no /root/reference)")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _run_pair(task, max_steps, extra, n, steps, seed, threads=3, stats=None):
    port = Oracle(task, n, seed=seed, max_episode_steps=max_steps, extra=extra, kind="port")
    ref = Oracle(task, n, seed=seed, max_episode_steps=max_steps, extra=extra,
                 kind="reference_mujoco", num_threads=threads)
    assert ref.kind == "reference_mujoco"
    assert port.keys == ref.keys
    assert (port.action_dtype, port.action_elems) == (ref.action_dtype, ref.action_elems)
    rng = np.random.default_rng(seed)
    a, b = port.reset(), ref.reset()
    dones = resets = 0
    for t in range(steps + 1):
        for k in a:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), (task, t, k, a[k].ravel()[:8], b[k].ravel()[:8])
        dones += int(a["done"].sum())
        resets += int((a["elapsed_step"] == 0).sum())
        if stats is not None:  # per-step outputs for the caller's checks of what the run exercised
            for k in a:
                stats.setdefault(k, []).append(a[k].copy())
        act = rng.uniform(-1.0, 1.0, size=(n, port.action_elems))
        a, b = port.step(act), ref.step(act)
    return dones, resets


@pytest.mark.parametrize("name", sorted(GYM_VARIANTS))
def test_task_restatement_is_the_reference_wrapper_bit_for_bit(name):
    task, max_steps, over = GYM_VARIANTS[name]
    dones, resets = _run_pair(task, max_steps, mj_extra(task, **over), n=6, steps=320, seed=11)
    # every task either terminates or truncates inside 320 steps except the 1000-step ones that
    # cannot fall; the auto-reset rows (elapsed_step == 0 after the initial reset) are compared too
    if max_steps <= 100 or task in ("Walker2d", "Walker2dV5", "Hopper", "InvertedPendulum",
                                    "InvertedDoublePendulum", "Humanoid"):
        assert dones > 0 and resets > 6


@pytest.mark.parametrize("name", ["HalfCheetah-v4", "Ant-v4", "Humanoid-v4"])
def test_short_episodes_truncate_like_the_reference(name):
    task, _, over = GYM_VARIANTS[name]
    dones, resets = _run_pair(task, 7, mj_extra(task, **over), n=5, steps=40, seed=2)
    assert dones >= 5 * 5


@pytest.mark.parametrize("name,over", [
    ("HalfCheetah-v4", dict(ctrl_cost_weight=0.3, forward_reward_weight=2.0, reset_noise_scale=0.03, frame_skip=3)),
    ("Ant-v4", dict(ctrl_cost_weight=0.1, reset_noise_scale=0.2, use_contact_force=1, post_constraint=1)),
    ("Pusher-v4", dict(dist_cost_weight=2.0, near_cost_weight=0.25, weighted_reward_info=1)),
    ("Hopper-v4", dict(legacy_healthy_reward=0, frame_skip=2)),
])
def test_non_default_options(name, over):
    task, max_steps, base = GYM_VARIANTS[name]
    _run_pair(task, max_steps, mj_extra(task, **{**base, **over}), n=4, steps=150, seed=5)


@pytest.mark.parametrize("case", sorted(MJ_OPTION_CASES))
def test_task_options_are_the_reference_config(case):
    """Every option of the MJ_OPTION_CASES table (tests/mj_util.py) through positions 25.. of `extra`
    against the same option set in the reference's config, bit for bit; the run must exercise what the
    case is about (terminations, their absence, clamps, resets)."""
    task, max_steps, extra, _, _, _, expect = option_case(case)
    lib = ctypes.CDLL(orc.REF_MUJOCO_LIB)
    if not hasattr(lib, "ref_mujoco_extra_positions") or lib.ref_mujoco_extra_positions() < len(extra):
        pytest.skip("oracle/_ref/libref_mujoco.so predates positions 25.. of `extra` (rebuild: make -C oracle ref)")
    opts = MJ_OPTION_CASES[case][2]
    humanoid = task.startswith("Humanoid")
    n, steps = (3, 40) if humanoid else (6, 150)
    st = {}
    _run_pair(task, max_steps, extra, n=n, steps=steps, seed=13, stats=st)
    done, trunc = np.stack(st["done"]).reshape(-1, n), np.stack(st["trunc"]).reshape(-1, n)
    elapsed = np.stack(st["elapsed_step"]).reshape(-1, n)
    obs = np.stack(st["obs"])
    terms = int((done & ~trunc).sum())
    resets = int((elapsed[1:] == 0).sum())  # auto-resets after the initial one
    assert resets >= n, (case, resets)
    if expect == "term":
        assert terms >= n, (case, terms)
    else:
        assert terms == 0 and trunc.any(), (case, terms)
    stepped = elapsed[1:] > 0
    if opts.get("exclude_current_positions_from_observation") == 0 and task not in ("Ant",) and not humanoid:
        # the planar root's x (Swimmer: x, y) leads the row: it is info:x_position of every step row
        x = np.stack(st["info:x_position"]).reshape(-1, n)[1:]
        assert np.array_equal(obs[1:, :, 0][stepped], x[stepped]), case
    if "contact_force_max" in opts:  # the clamp of the contact-force observation is active
        assert (np.abs(obs[..., -78:]) == opts["contact_force_max"]).sum() > 100, case
    if "contact_cost_max" in opts:  # the clamp of the contact cost is active
        impact = np.stack(st["info:reward_impact"])
        assert (impact == -opts["contact_cost_max"]).sum() > n, case
    if "observation_max" in opts:
        assert (np.abs(obs[..., 5:]) == opts["observation_max"]).sum() > n, case
    alive_key = {"Ant": "info:reward_survive", "Humanoid": "info:reward_alive"}.get(task)
    if alive_key:
        alive = np.stack(st[alive_key]).reshape(-1, n)[1:]
        hr = opts.get("healthy_reward", 1.0 if task == "Ant" else 5.0)
        if expect == "noterm":  # paid only while healthy: the run has both
            assert (alive[stepped] == 0).any() and (alive[stepped] == hr).any(), case
        else:  # the terminal step: paid under the legacy rule only
            legacy = {**GYM_VARIANTS[MJ_OPTION_CASES[case][0]][2], **opts}.get("legacy_healthy_reward", 1)
            term = (done & ~trunc)[1:]
            assert (alive[term] == (hr if legacy else 0.0)).all(), case


def test_partial_id_sends_and_reset_subsets():
    """Send() for a subset of ids and Reset(ids) mid-episode (mujoco_gym_envpool_test.cc shape)."""
    task, ms, over = GYM_VARIANTS["Walker2d-v4"]
    ex = mj_extra(task, **over)
    n = 8
    port = Oracle(task, n, seed=9, max_episode_steps=ms, extra=ex, kind="port")
    ref = Oracle(task, n, seed=9, max_episode_steps=ms, extra=ex, kind="reference_mujoco", num_threads=2)
    rng = np.random.default_rng(1)
    a, b = port.reset(), ref.reset()
    for t in range(60):
        ids = np.sort(rng.choice(n, size=int(rng.integers(1, n + 1)), replace=False)).astype(np.int32)
        act = rng.uniform(-1, 1, size=(len(ids), port.action_elems))
        if t % 17 == 5:
            a, b = port.reset(ids), ref.reset(ids)
        else:
            a, b = port.step(act, ids), ref.step(act, ids)
        for k in a:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), (t, k)


def test_frame_stack_is_the_reference_ring():
    """frame_stack=3 through the reference's own FrameStackBuffer (envpool/mujoco/frame_stack.h)
    equals stacking the restatement's single frames: reset fills every slot, a step shifts."""
    task, ms, over = GYM_VARIANTS["HalfCheetah-v4"]
    n, fs = 3, 3
    port = Oracle(task, n, seed=4, max_episode_steps=9, extra=mj_extra(task, **over), kind="port")
    ref = Oracle(task, n, seed=4, max_episode_steps=9, extra=mj_extra(task, frame_stack=fs, **over),
                 kind="reference_mujoco")
    assert dict((k, e) for k, _, e in ref.keys)["obs"] == fs * 17
    rng = np.random.default_rng(0)
    a, b = port.reset(), ref.reset()
    ring = np.repeat(a["obs"][:, None, :], fs, axis=1)
    for t in range(30):
        assert np.array_equal(_bits(ring.reshape(n, -1)), _bits(b["obs"])), t
        act = rng.uniform(-1, 1, size=(n, 6))
        a, b = port.step(act), ref.step(act)
        for e in range(n):
            if a["elapsed_step"][e, 0] == 0:
                ring[e] = a["obs"][e]
            else:
                ring[e] = np.concatenate([ring[e, 1:], a["obs"][e][None]], axis=0)


# every body of the reference's *_envpool.xml files in document order, world first (tools/mjcf_subset.py's reading;
# tests/test_models_vs_xml.py::test_golden_is_what_the_xml_says pins it to the XML where the reference tree exists)
MJCF_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mjcf_models.json")


@pytest.mark.parametrize("xml,bodies", [
    ("ant", ["torso"]),
    ("reacher", ["fingertip", "target"]),
    ("pusher", ["tips_arm", "object", "goal"]),
    ("pusher_v5", ["tips_arm", "object", "goal"]),
])
def test_body_ids_are_the_xml_document_order(xml, bodies):
    """mj_name2id of the shim == MuJoCo's rule (body ids in document order, world = 0),
    the order read from the reference's XML (tests/golden/mjcf_models.json)."""
    with open(MJCF_GOLDEN) as f:
        names = [b["name"] for b in json.load(f)[xml]["bodies"]]
    assert names[0] == "world"
    order = names[1:]
    lib = ctypes.CDLL(orc.REF_MUJOCO_LIB)
    lib.ref_mujoco_body_id.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    assert lib.ref_mujoco_nbody((xml + ".xml").encode()) == len(order) + 1
    for b in bodies:
        assert lib.ref_mujoco_body_id((xml + ".xml").encode(), b.encode()) == order.index(b) + 1
