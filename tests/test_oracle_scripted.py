"""Pin the plain-C oracle (oracle/restate) at the branches random play never takes.

(a) bit for bit against the scripted rollouts of the reference (tests/golden/scripted_*.npz, made by
    tests/golden/make_scripted_golden.py from the policies of tests/scripted_cases.py), replayed open loop;
(b) the committed files still contain the events they exist for;
(c) bit for bit against oracle/_ref under the same policies, closed loop, with another seed and more envs, whenever
    that library is present;
(d) the one-step lattices and tables that the GPU tests step through the kernels (tests/classic_edge_rows.py,
    tests/toy_edge_rows.py): on the port alone, every crafted row takes the side of its decision that it was placed
    on, and the discrete-state hook of the port agrees with the reference's own trajectories.
"""
import os

import numpy as np
import pytest

import classic_edge_rows as cer
import toy_edge_rows as ter
from oracle.orc import Oracle, have_ref
from scripted_cases import LIVE_SEED, SCRIPTED, check_events, rollout
from test_oracle_pinned import GOLDEN, replay_golden


def scripted_port(name):
    c = SCRIPTED[name]
    return lambda n, seed: Oracle(c["task"], n, seed=seed, max_episode_steps=c["max_steps"], extra=c["extra"],
                                  kind="port")


@pytest.mark.parametrize("name", sorted(SCRIPTED))
def test_port_matches_scripted_golden(name):
    for key, want, got in replay_golden(scripted_port(name), "scripted_" + name):
        assert got.dtype == want.dtype, key
        assert np.array_equal(got, want), f"{name}:{key} differs from reference"


@pytest.mark.parametrize("name", sorted(SCRIPTED))
def test_scripted_golden_holds_its_events(name):
    g = np.load(os.path.join(GOLDEN, "scripted_" + name + ".npz"))
    assert g["actions"].shape[:2] == (SCRIPTED[name]["T"], 8)
    counts = check_events(name, g)
    print(name, counts)


@pytest.mark.skipif(not have_ref(), reason="oracle/_ref not built here")
@pytest.mark.parametrize("name", sorted(SCRIPTED))
def test_port_matches_compiled_reference_under_policy(name):
    c = SCRIPTED[name]
    n = 16
    ref = Oracle(c["task"], n, seed=LIVE_SEED, max_episode_steps=c["max_steps"], extra=c["extra"],
                 kind="reference", num_threads=2)
    port = Oracle(c["task"], n, seed=LIVE_SEED, max_episode_steps=c["max_steps"], extra=c["extra"], kind="port")
    assert [k[:2] for k in ref.keys] == [k[:2] for k in port.keys]
    a, b = rollout(ref, c, n, follower=port)
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (name, k)


# ---- (d) the one-step lattices on the port alone ---------------------------------------------------------------
def port_lattice_step(name):
    """The port's frame and fp64 state after one step from the lattice's rows."""
    task, version, rows = cer.lattice(name)
    port = Oracle(task, cer.N_ROWS, seed=5, max_episode_steps=cer.LIMIT, extra=(version,), kind="port")
    port.reset()
    port.set_state(cer.flat_state(rows, 5))
    frame = port.step(rows["action"])
    return rows, frame, port.get_state()


@pytest.mark.parametrize("name", sorted(cer.LATTICES))
def test_lattice_rows_sit_where_they_were_placed(name):
    rows, frame, post = port_lattice_step(name)
    assert cer.N_ROWS % 64 != 0
    assert rows["groups"]
    for group, sl, expect in rows["groups"]:
        ok = expect(post[sl], {k: v[sl] for k, v in frame.items()})
        assert ok.all(), (name, group, np.nonzero(~ok)[0][:8])
    # the step limit meets a threshold crossing in the same row
    both = frame["done"][:, 0] & frame["trunc"][:, 0]
    assert both.any()
    if not name.startswith("Pendulum"):  # (Pendulum ends at the step limit only)
        assert (frame["done"][:, 0] & ~frame["trunc"][:, 0]).any()
    if "stats" in rows:  # Acrobot: sampled densely, rows with a margin below DELTA dropped
        stats = dict(rows["stats"])
        print(name, stats)
        assert stats.pop("dropped") <= 0.01
        stats.pop("placed")
        for decision, (taken, not_taken, taken_close, not_taken_close) in stats.items():
            assert taken >= 32 and not_taken >= 32, (decision, taken, not_taken)
            # and within 3 DELTA of the threshold on either side: the rows that a float32 decision gets wrong
            if decision in cer.ACROBOT_PLACED:
                assert taken_close >= 32 and not_taken_close >= 32, (decision, taken_close, not_taken_close)


# ---- (d) the discrete-state hook --------------------------------------------------------------------------------
HOOK_FIXTURES = {
    "Taxi": ("scripted_taxi_script", 200), "CliffWalking": ("scripted_cliffwalking_paths", 0),
    "CliffWalkingSlippery": ("scripted_cliffwalking_slippery", 0), "FrozenLake4x4": ("scripted_frozenlake_goal", 100),
    "FrozenLake8x8": ("scripted_frozenlake8x8_goal", 200), "NChain": ("scripted_nchain_hold", 1000),
    "Catch10x5": ("Catch-v0", 0),
}


@pytest.mark.parametrize("name", sorted(HOOK_FIXTURES))
def test_discrete_state_hook_follows_the_reference(name):
    """Along a rollout of the reference, the port's discrete state read through the hook packs to the recorded
    observation, and writing it back before every step changes nothing: the exhaustive tables of the GPU tests set
    states through this hook and this packing."""
    fixture, max_steps = HOOK_FIXTURES[name]
    task, extra, _, _, _, _ = ter.TABLES[name]
    ncols = len(ter.TABLES[name][3])
    g = np.load(os.path.join(GOLDEN, fixture + ".npz"))
    n = g["actions"].shape[1]
    port = Oracle(task, n, seed=int(g["seed"]), max_episode_steps=max_steps, extra=extra, kind="port")
    frame = port.reset()
    for t in range(g["actions"].shape[0] + 1):
        st = port.get_discrete()
        obs = g["state/obs"][t].reshape(n, -1)
        assert np.array_equal(frame["obs"].reshape(n, -1), obs), (name, t)
        assert np.array_equal(st[:, 12], frame["done"][:, 0]) and np.array_equal(st[:, 13], frame["elapsed_step"][:, 0])
        if task == "Catch":
            x, y, paddle = st[:, 0], st[:, 1], st[:, 2]
            want = np.zeros_like(obs)
            want[np.arange(n), x * 5 + y] = 1
            want[np.arange(n), 9 * 5 + paddle] = 1
            assert np.array_equal(want, obs), (name, t)
        else:
            assert np.array_equal(ter.pack(name, st[:, :ncols]), obs[:, 0]), (name, t)
        if t == g["actions"].shape[0]:
            break
        port.set_discrete(st)
        frame = port.step(g["actions"][t])


def test_toy_tables_cover_every_state_and_action():
    for name, (task, _, _, ranges, n_act, repeat) in ter.TABLES.items():
        tb = ter.table(name)
        assert tb["n"] == int(np.prod(ranges)) * (n_act + 3) * repeat
        pairs = set(zip(ter.pack(name, tb["cols"]).tolist(), tb["action"].tolist()))
        assert len(pairs) == int(np.prod(ranges)) * (n_act + 3), name
        assert {-1, n_act, n_act + 1} <= set(tb["action"].tolist())
        lim = tb["cur"] == ter.LIMIT - 1
        assert len(set(zip(ter.pack(name, tb["cols"])[lim].tolist(), tb["action"][lim].tolist()))) >= len(pairs) // 5
    assert ter.table("Taxi")["n"] == 500 * 9 and ter.table("CliffWalking")["n"] == 48 * 7
