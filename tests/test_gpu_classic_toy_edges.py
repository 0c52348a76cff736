"""GPU parity of classic_control and toy_text at the branches random play never takes.

(a) the scripted rollouts of the reference (tests/golden/scripted_*.npz) through the kernels: toy_text bit exact;
    classic_control free running at the bar of test_classic_golden_rollout, and teacher-forced from the port's fp64
    state along the scripted trajectory at the 4 ulp(fp32) of test_classic_teacher_forced;
(b) one-step boundary lattices of crafted fp64 states (tests/classic_edge_rows.py) against the port;
(c) exhaustive one-step tables of toy_text (tests/toy_edge_rows.py) against the port, bit exact.
classic_control runs in both forms of ClassicStepKernel ("classic_early" 0 and 1).
"""
import numpy as np
import pytest

import classic_edge_rows as cer
import toy_edge_rows as ter
from envpool_amd.core.device_pool import DevicePool
from hip_util import PARAM_NAMES, HipAsOracle
from oracle.orc import Oracle
from scripted_cases import SCRIPTED, SCRIPTED_CLASSIC, SCRIPTED_TOY
from test_gpu_classic_toy import ulp_diff_f32
from test_oracle_pinned import GOLDEN, replay_golden

pytestmark = pytest.mark.gpu

EXACT_KEYS = ("done", "trunc", "elapsed_step", "step_type")


def scripted_pool(name, n, seed, **engine_keys):
    c = SCRIPTED[name]
    params = dict(zip(PARAM_NAMES.get(c["task"], ()), c["extra"]))
    params.update(engine_keys)
    return DevicePool(c["task"], n, seed=seed, max_episode_steps=c["max_steps"], params=params)


def assert_float_rows(got, want, what):
    """float32 rows within 4 ulp, compared by bits with NaN equal to NaN."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    d = ulp_diff_f32(np.where(nan, 0, got), np.where(nan, 0, want))
    assert d.max() <= 4, (what, int(d.max()), np.argwhere(d > 4)[:4].tolist())
    return int(d.max())


# ---- (a) scripted fixtures ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCRIPTED_TOY)
def test_toy_text_scripted_golden(name):
    def make(n, seed):
        return HipAsOracle(scripted_pool(name, n, seed))

    for key, want, got in replay_golden(make, "scripted_" + name):
        assert got.dtype == want.dtype, key
        assert np.array_equal(got, want), f"{name}:{key}"


@pytest.mark.parametrize("early", [0, 1])
@pytest.mark.parametrize("name", SCRIPTED_CLASSIC)
def test_classic_scripted_golden_rollout(name, early):
    """Free running against the reference's scripted rollout: done, trunc, elapsed_step and step_type exact for the
    whole rollout, and every key of every reset row; float keys within 1e-5 rel for the first 51 rows."""
    def make(n, seed):
        return HipAsOracle(scripted_pool(name, n, seed, classic_early=early))

    g = np.load(GOLDEN + "/scripted_" + name + ".npz")
    reset_rows = g["state/elapsed_step"].reshape(g["state/elapsed_step"].shape[:2]) == 0
    for key, want, got in replay_golden(make, "scripted_" + name):
        assert got.dtype == want.dtype, key
        if key in EXACT_KEYS:
            assert np.array_equal(got, want), f"{name}:{key}"
        assert np.array_equal(got[reset_rows], want[reset_rows]), f"{name}:{key} reset rows"
        if want.dtype == np.float32:
            np.testing.assert_allclose(got[:51], want[:51], rtol=1e-5, atol=1e-6, err_msg=f"{name}:{key}")
        else:
            assert np.array_equal(got[:51], want[:51]), f"{name}:{key}"


@pytest.mark.parametrize("early", [0, 1])
@pytest.mark.parametrize("name", SCRIPTED_CLASSIC)
def test_classic_scripted_teacher_forced(name, early):
    """Along the scripted trajectory of the port (= the reference's, test_port_matches_scripted_golden), the pool is
    set to the port's fp64 state before every step: integer keys exact, float keys within 4 ulp(fp32)."""
    c = SCRIPTED[name]
    g = np.load(GOLDEN + "/scripted_" + name + ".npz")
    acts = g["actions"]
    n, seed = acts.shape[1], int(g["seed"])
    pool = scripted_pool(name, n, seed, classic_early=early)
    hip = HipAsOracle(pool)
    orc = Oracle(c["task"], n, seed=seed, max_episode_steps=c["max_steps"], extra=c["extra"], kind="port")
    a, b = hip.reset(), orc.reset()
    for k in b:
        assert np.array_equal(a[k], b[k]), (name, "reset", k)
    ns = cer.NS[c["task"]]
    worst = 0
    for t in range(acts.shape[0]):
        st = orc.get_state()  # [s0..s4, done, cur_step]
        pool.set_state(np.concatenate([st[:, :ns], st[:, 5:7]], axis=1))
        a, b = hip.step(acts[t]), orc.step(acts[t])
        for k in b:
            if b[k].dtype == np.float32:
                worst = max(worst, assert_float_rows(a[k], b[k], (name, t, k)))
            else:
                assert np.array_equal(a[k], b[k]), (name, t, k)
    print(f"{name} early={early}: worst teacher-forced diff along the scripted rollout = {worst} ulp(fp32)")


# ---- (b) one-step boundary lattices ------------------------------------------------------------------------------
@pytest.mark.parametrize("early", [0, 1])
@pytest.mark.parametrize("name", sorted(cer.LATTICES))
def test_classic_boundary_lattice(name, early):
    """One step from every row of the lattice, kernel against port: integer and bool keys exact, float obs and reward
    within 4 ulp(fp32) (NaN equal to NaN); and the fp64 state the step leaves, which is where a clamp or a wrap
    taken on the wrong side of a DELTA = 1e-9 margin shows (float32 observations cannot resolve it): within 1e-10.
    A last-bit difference of sin / cos (1e-16) reaches the state through at most Acrobot's RK4 step, times
    velocities squared of up to 3e3 and a handful of operations: some 1e-12; 1e-10 is a tenth of DELTA."""
    task, version, rows = cer.lattice(name)
    n = cer.N_ROWS
    params = {"classic_early": early}
    if task == "Pendulum":
        params["version"] = version
    pool = DevicePool(task, n, seed=5, max_episode_steps=cer.LIMIT, params=params)
    hip = HipAsOracle(pool)
    orc = Oracle(task, n, seed=5, max_episode_steps=cer.LIMIT, extra=(version,), kind="port")
    hip.reset(), orc.reset()
    ns = cer.NS[task]
    pool.set_state(cer.flat_state(rows, ns))
    orc.set_state(cer.flat_state(rows, 5))
    a, b = hip.step(rows["action"]), orc.step(rows["action"])
    worst = 0
    for k in b:
        if b[k].dtype == np.float32:
            worst = max(worst, assert_float_rows(a[k], b[k], (name, k)))
        else:
            assert np.array_equal(a[k], b[k]), (name, k, np.nonzero((a[k] != b[k]).any(axis=1))[0][:8])
    post_hip, post_orc = pool.get_state(), orc.get_state()
    assert np.array_equal(post_hip[:, ns:], post_orc[:, 5:7]), name
    sa, sb = post_hip[:, :ns], post_orc[:, :ns]
    assert np.array_equal(np.isnan(sa), np.isnan(sb)), name
    diff = np.abs(np.where(np.isnan(sb), 0, sa - sb))
    assert diff.max() <= 1e-10, (name, float(diff.max()), np.argwhere(diff > 1e-10)[:4].tolist())
    print(f"{name} early={early}: worst diff {worst} ulp(fp32), fp64 state {diff.max():.3g}")


# ---- (c) exhaustive one-step tables ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ter.TABLES))
def test_toy_text_exhaustive_step_table(name):
    """Every state x every action (and -1, n, n + 1) in one pool and one step, bit exact on every key against the
    port, and the state the step leaves.  Both sides are reset with the same seeds first, so their generators stand
    at the same word for the slip draws."""
    tb = ter.table(name)
    n = tb["n"]
    pool = DevicePool(tb["task"], n, seed=9, max_episode_steps=ter.LIMIT, params=tb["params"])
    hip = HipAsOracle(pool)
    orc = Oracle(tb["task"], n, seed=9, max_episode_steps=ter.LIMIT, extra=tb["extra"], kind="port")
    a, b = hip.reset(), orc.reset()
    for k in b:
        assert np.array_equal(a[k], b[k]), (name, "reset", k)
    pool.set_state(tb["kernel_state"])
    orc.set_discrete(tb["istate"])
    a, b = hip.step(tb["action"]), orc.step(tb["action"])
    for k in b:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), \
            (name, k, np.nonzero((a[k] != b[k]).any(axis=1))[0][:8])
    assert b["done"].any() and (b["done"] & b["trunc"]).any() and not b["trunc"].all()
    post_hip, post_orc = pool.get_state(), orc.get_discrete()
    assert np.array_equal(post_hip[:, 0], ter.pack(name, post_orc[:, :tb["ncols"]])), name
    assert np.array_equal(post_hip[:, 2:4], post_orc[:, 12:14]), name
