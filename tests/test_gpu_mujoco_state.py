"""The flat state hooks (state_dim / get_state / set_state) of the gym-MuJoCo pools, family by family.

Flat layout, the one oracle/mjcpu uses: qpos[nq] qvel[nv] warm[nv] | time xlag ylag done cur_step
normal_saved normal_avail, and for the Pusher five more lag values behind it.  What a family stores:
  slot 0 (time)        nobody: get_state only ever writes it (0 on a fresh pool; HalfCheetah / Walker2d / Hopper
                       and the Ant report solver counters of the last step there)
  slots 1, 2 (lag)     Reacher, Ant, Humanoid, HumanoidStandup; the Pusher takes its five lag rows from the
                       appended block and get_state mirrors the first two of them into slots 1, 2
  slots 3, 4           done (!= 0) and cur_step (int), every family
  slots 5, 6           the saved normal variate and its flag (!= 0): the planar robots, Ant, the pendulums, Swimmer
Every other slot reads 0 and is ignored on set_state.

num_envs = 40 is no multiple of 16 or 64: the last lane-group chunk and the last wave are partial."""
import numpy as np
import pytest

from envpool_amd.core.device_pool import DevicePool
from tests.mj_util import native_variant

pytestmark = pytest.mark.gpu

N = 40
IDS = np.array([39, 0, 17, 16, 15, 3], dtype=np.int32)

# case -> (registered id, engine keys, nq, nv, lag in slots 1 / 2, normal pair, appended lag rows, state_dim)
CASES = {
    "HalfCheetah": ("HalfCheetah-v4", {}, 9, 9, False, True, 0, 34),
    "Walker2d": ("Walker2d-v4", {}, 9, 9, False, True, 0, 34),
    "Hopper-layout0": ("Hopper-v4", {"planar_layout": 0}, 6, 6, False, True, 0, 25),
    "Hopper-layout1": ("Hopper-v4", {"planar_layout": 1}, 6, 6, False, True, 0, 25),
    "Ant": ("Ant-v4", {}, 15, 14, True, True, 0, 50),
    "Swimmer": ("Swimmer-v4", {}, 5, 5, False, True, 0, 22),
    "Reacher": ("Reacher-v4", {}, 4, 4, True, False, 0, 19),
    "Pusher": ("Pusher-v4", {}, 11, 11, False, False, 5, 45),
    "InvertedPendulum": ("InvertedPendulum-v4", {}, 2, 2, False, True, 0, 13),
    "InvertedDoublePendulum": ("InvertedDoublePendulum-v4", {}, 3, 3, False, True, 0, 16),
    "Humanoid": ("Humanoid-v4", {}, 24, 23, True, False, 0, 77),
    "HumanoidStandup": ("HumanoidStandup-v4", {}, 24, 23, True, False, 0, 77),
}
_AMAX = {"InvertedPendulum": 3.0, "Pusher": 2.0, "Humanoid": 0.4, "HumanoidStandup": 0.4}


def _pool(case):
    gym_id, keys = CASES[case][:2]
    family, max_steps, params = native_variant(gym_id)
    return DevicePool(family, N, seed=11, max_episode_steps=max_steps, params={**params, **keys})


def _random_state(case, seed):
    _, _, nq, nv, _, _, extra, dim = CASES[case]
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((N, dim))
    t = nq + 2 * nv
    s[:, t + 3] = rng.integers(0, 2, N)   # done
    s[:, t + 4] = rng.integers(0, 50, N)  # cur_step
    s[:, t + 6] = rng.integers(0, 2, N)   # normal_avail
    return s


def _stored(case, s):
    """What get_state returns after set_state(s) on a fresh pool."""
    _, _, nq, nv, lag, normal, extra, dim = CASES[case]
    t = nq + 2 * nv
    assert dim == t + 7 + extra
    g = np.zeros_like(s)
    g[:, :t] = s[:, :t]
    g[:, t + 3:t + 5] = s[:, t + 3:t + 5]
    if lag:
        g[:, t + 1:t + 3] = s[:, t + 1:t + 3]
    if normal:
        g[:, t + 5:t + 7] = s[:, t + 5:t + 7]
    if extra:
        g[:, t + 7:] = s[:, t + 7:]
        g[:, t + 1:t + 3] = s[:, t + 7:t + 9]  # the mirror of lag rows 0, 1
    return g


def _same_bits(a, b, tag):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (tag, a.shape, b.shape, a.dtype, b.dtype)
    bad = np.argwhere(a.view(np.uint8) != b.view(np.uint8))
    assert bad.size == 0, (tag, bad[:4].tolist())


@pytest.mark.parametrize("case", sorted(CASES))
def test_set_then_get_on_a_fresh_pool(case):
    pool = _pool(case)
    assert pool.state_dim() == CASES[case][7]
    s = _random_state(case, 1)
    assert np.isfinite(s).all()
    pool.set_state(s)
    _same_bits(pool.get_state(), _stored(case, s), case)
    pool.close()


@pytest.mark.parametrize("case", sorted(CASES))
def test_subset_and_order(case):
    pool = _pool(case)
    s0, s1 = _random_state(case, 2), _random_state(case, 3)
    pool.set_state(s0)
    pool.set_state(s1[IDS], IDS)
    want = _stored(case, s0)
    want[IDS] = _stored(case, s1)[IDS]
    _same_bits(pool.get_state(), want, case)
    _same_bits(pool.get_state(IDS), want[IDS], case + " ids")
    pool.close()


@pytest.mark.parametrize("case", sorted(CASES))
def test_view_aliases_what_the_kernels_step(case):
    family = native_variant(CASES[case][0])[0]
    rng = np.random.default_rng(4)
    ids = np.arange(N, dtype=np.int32)

    def actions(pool):
        return rng.uniform(-1.0, 1.0, size=(N, *pool.action_shape)) * _AMAX.get(family, 1.0)

    src = _pool(case)  # a valid configuration: a reset plus two steps (random qpos is none)
    src.reset(ids)
    src.recv()
    for _ in range(2):
        src.send(ids, actions(src))
        src.recv()
    valid = src.get_state()
    src.close()

    a, b = _pool(case), _pool(case)
    a.set_state(valid)
    perm = np.random.default_rng(5).permutation(N).astype(np.int32)
    for part in (perm[:23], perm[23:]):
        b.set_state(valid[part], part)
    act = actions(a)
    a.send(ids, act)
    b.send(ids, act)
    ra, rb = a.recv_dict(), b.recv_dict()
    assert list(ra) == list(rb)
    for key in ra:
        _same_bits(ra[key], rb[key], f"{case} {key}")
    ga, gb = a.get_state(), b.get_state()
    t = CASES[case][2] + 2 * CASES[case][3]
    live = valid[:, t + 3] == 0  # the step continued the episode set_state put there
    assert live.any() and (ga[live, t + 4] == valid[live, t + 4] + 1).all()
    if family == "Ant":  # slot 0: per-step profiling counters
        ga[:, t] = gb[:, t] = 0.0
    _same_bits(ga, gb, case + " state")
    a.close()
    b.close()
