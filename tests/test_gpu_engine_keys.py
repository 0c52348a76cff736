"""The engine keys that are documented to change speed only (include/envpool_amd.h, "Never changes results"): a pool
built with such a key set returns, bit for bit in every key of every row, what a pool of the same seed returns with the
key at its other value.

  mt_tile        every step kernel in both generator layouts, the generators carried across word 623 -> 0
  classic_block, classic_rows, classic_early   every launch shape of the classic_control step kernel, ragged last trip
  planar_lpt, copy_threads, numa_bind          see the tests"""
import numpy as np
import pytest

from test_gpu_snapshot import TASKS, Handle, blob_generators, same_bits, same_rows

pytestmark = pytest.mark.gpu

N = 40
SNAP_EVERY = 4  # steps between two looks at the generator positions

# case -> (max_episode_steps, steps, the run carries every env's generator across word 623 -> 0).
# Per env a reset falls every max_episode_steps + 1 sends at the latest (the send after `done` is the reset), so
# `steps` sends hold at least steps // (max_episode_steps + 1) resets, and the run wraps when these resets and what
# the steps draw make more than 624 words: CartPole 8 words per reset (100 resets: 800 words), Pendulum 4 (165
# resets: 660), the Hopper 24, Humanoid 94; the others draw a number of words that varies (rejection loops, the polar
# method of the normal draws, cards, spawned tiles, shuffles, moving obstacles), and their steps are sized from the
# fewest words any of the 40 envs drew in such a run, with a margin: HalfCheetah 13 per send, the Ant 20,
# InvertedDoublePendulum, Reacher and Blackjack and Game2048 a little over 2 to 4, Pusher 6.5, Minesweeper 10, the
# MiniGrid ids 6 and 13.  The test itself checks that every env wrapped.
# Compared WITHOUT a wrap, because they cannot draw 624 words per env in about 300 steps: FrozenLake (one word per
# step, none per reset), Snake (a draw only for a new fruit), Othello and Hex (the reset draws the player order only).
WRAP_PLAN = {
    "CartPole-v1": (2, 300, True),
    "Pendulum-v1": (1, 330, True),
    "Blackjack-v1": (6, 340, True),
    "FrozenLake8x8-v1": (7, 300, False),
    "HalfCheetah-v4": (2, 75, True),
    "Hopper-v4/planar_layout=0": (2, 96, True),
    "Hopper-v4/planar_layout=1": (2, 96, True),
    "Ant-v4": (2, 48, True),
    "InvertedDoublePendulum-v4": (2, 200, True),
    "Reacher-v4": (2, 180, True),
    "Pusher-v4": (2, 120, True),
    "Humanoid-v4": (2, 30, True),
    "MiniGrid-Dynamic-Obstacles-6x6-v0": (6, 100, True),
    "MiniGrid-DoorKey-5x5-v0": (2, 150, True),
    "Game2048-v1": (6, 330, True),
    "Snake-v1": (6, 300, False),
    "Minesweeper-v0": (2, 90, True),
    "Othello-v1": (7, 300, False),
    "Hex-v1": (7, 300, False),
}
assert set(WRAP_PLAN) == set(TASKS)


def positions(h, shift):
    got, mti = blob_generators(h.pool.snapshot())
    assert got == shift  # (the key has reached the engine)
    return mti


def both_layouts(case, max_episode_steps, steps, seed=11):
    """Two pools of one seed, generators [624][N] and tiled, stepped with the same actions: every row alike, the
    generator positions alike.  Returns per pool and env whether its position went down between two looks."""
    pools = [Handle(case, seed=seed, engine_keys={"mt_tile": t}, max_episode_steps=max_episode_steps) for t in (1, 16)]
    rng = np.random.default_rng(2)
    first = [h.reset() for h in pools]
    same_rows([first[1]], [first[0]], (case, "reset"))
    prev = [positions(h, s) for h, s in zip(pools, (0, 4))]
    wrapped = [np.zeros(N, bool), np.zeros(N, bool)]
    for t in range(steps):
        act = pools[0].actions(rng)
        rows = [h.step(act) for h in pools]
        same_rows([rows[1]], [rows[0]], (case, t))
        if t % SNAP_EVERY == SNAP_EVERY - 1 or t == steps - 1:
            now = [positions(h, s) for h, s in zip(pools, (0, 4))]
            same_bits(now[1], now[0], (case, t, "generator positions"))
            for i in range(2):
                wrapped[i] |= now[i] < prev[i]
            prev = now
    for h in pools:
        h.close()
    return wrapped


@pytest.mark.parametrize("case", sorted(TASKS))
def test_both_generator_layouts_step_alike(case):
    """"mt_tile" 1 against 16 for one id per step kernel.  Where WRAP_PLAN says so the run is long enough for every
    env to pass word 623 -> 0 at least once in both pools (where the tiled layout regenerates its first tile out of
    the last one's neighbour word and the partner words change sides), and the test checks that it did: a position
    that goes down between two looks SNAP_EVERY steps apart is a wrap (no env draws 624 words in four steps).
    Without a wrap: FrozenLake, Snake, Othello, Hex (see WRAP_PLAN)."""
    max_episode_steps, steps, wraps = WRAP_PLAN[case]
    wrapped = both_layouts(case, max_episode_steps, steps)
    if wraps:
        assert wrapped[0].all() and wrapped[1].all(), (case, np.flatnonzero(~wrapped[0]), np.flatnonzero(~wrapped[1]))


@pytest.mark.parametrize("tile", [0, 2, 8, 32])
def test_other_tile_widths_are_refused(tile):
    with pytest.raises(ValueError, match="mt_tile"):
        Handle("CartPole-v1", seed=1, engine_keys={"mt_tile": tile})


# ---- the launch shape of the classic_control step kernel ----------------------------------------
CLASSIC = ["CartPole-v1", "Pendulum-v1", "MountainCar-v0", "MountainCarContinuous-v0", "Acrobot-v1"]
CLASSIC_N = 1541   # no multiple of 64; block 64 x rows 8: 4 blocks, 6 or 7 trips per thread, the last one ragged
CLASSIC_PART = 517
SHAPES = [{"classic_block": b, "classic_rows": r, "classic_early": e}
          for b in (64, 128, 256) for r in (1, 3, 8) for e in (0, 1)]


def classic_pool(task, keys, n=CLASSIC_N):
    from hip_util import registered_pool

    return registered_pool(task, n, 23, keys, max_episode_steps=3)


def recv_rows(pool):
    d = pool.recv_dict()
    rows = len(d["info:env_id"])
    return {k: np.array(v).reshape(rows, -1) for k, v in d.items()}


@pytest.mark.parametrize("task", CLASSIC)
def test_classic_launch_shapes_step_alike(task):
    """Every "classic_block" x "classic_rows" x "classic_early" against the default keys: 40 steps of episodes of 3
    steps (resets in every trip of the grid-stride loop), every fifth send 517 ids out of order."""
    import envpool_amd as envpool

    pools = [classic_pool(task, None)] + [classic_pool(task, s) for s in SHAPES]
    sp = envpool.make_spec(task).action_space
    rng = np.random.default_rng(6)
    ids = np.arange(CLASSIC_N, dtype=np.int32)

    def everybody(send):
        for p in pools:
            send(p)
        rows = [recv_rows(p) for p in pools]
        for shape, r in zip(SHAPES, rows[1:]):
            same_rows([r], [rows[0]], (task, shape))
        return rows[0]

    everybody(lambda p: p.reset(ids))
    resets = 0
    for t in range(40):
        part = rng.permutation(CLASSIC_N)[:CLASSIC_PART].astype(np.int32) if t % 5 == 4 else ids
        if hasattr(sp, "n"):
            act = rng.integers(0, sp.n, len(part)).astype(pools[0].action_dtype)
        else:
            act = rng.uniform(sp.low, sp.high, (len(part), *sp.shape)).astype(pools[0].action_dtype)
        want = everybody(lambda p: p.send(part, act))
        same_bits(want["info:env_id"][:, 0], part, (task, t, "rows in send order"))
        resets += int((want["elapsed_step"] == 0).sum())
    assert resets >= 8 * CLASSIC_N  # (episodes of 3 steps: a reset every fourth send of an env)
    for p in pools:
        p.close()


@pytest.mark.parametrize("keys", [{"classic_block": 96}, {"classic_block": 32}, {"classic_rows": 0},
                                  {"classic_rows": 9}])
def test_other_classic_launch_shapes_are_refused(keys):
    with pytest.raises(ValueError, match="classic_block"):
        classic_pool("Pendulum-v1", keys, n=64)


# ---- the second trip of the default grid-stride loops -------------------------------------------
# ClassicStepKernel and ToyStepKernel launch at most 2048 blocks of 256 threads with the default keys: a pool of more
# than 524288 envs is the only way into the second trip of their loops (in ToyStepKernel it reuses the two LDS arrays
# behind Catch's cooperative observation stores), and 70 more rows make that trip a ragged one.
TRIP = 2048 * 256
BIG_N = TRIP + 70
BIG_TAIL = 256 + 70  # the last 256 rows of the first trip and all of the second


@pytest.mark.parametrize("name", ["Catch-v0", "FrozenLake-v1", "CartPole-v1"])
def test_second_trip_of_the_grid_stride_loop(name):
    """The last 326 envs of a pool of 524288 + 70 against the port oracle seeded seed + N - 326 (env i of a pool is
    seeded seed + i), free running for 12 steps (Catch's episodes take 9: an auto-reset in both trips): every key bit
    for bit, CartPole's float keys within 1e-5 relative as at the 65536-env size."""
    import time

    from hip_util import make_hip_pool
    from oracle.orc import Oracle
    from oracle_cases import CASES, INTEGER_EXACT, sample_actions

    t0 = time.time()
    c = CASES[name]
    exact = name in INTEGER_EXACT
    big = make_hip_pool(name, BIG_N, 3)
    orc = Oracle(c["task"], BIG_TAIL, seed=3 + BIG_N - BIG_TAIL, max_episode_steps=c["max_steps"], extra=c["extra"],
                 kind="port")
    ids = np.arange(BIG_N, dtype=np.int32)
    tail = slice(BIG_N - BIG_TAIL, BIG_N)
    rng = np.random.default_rng(4)
    big.reset(ids)
    a, o = big.recv_dict(), orc.reset()
    ends = 0
    for k in range(13):
        for key, want in o.items():
            got = a[key].reshape(BIG_N, -1)[tail]
            if key in ("info:env_id", "info:players.env_id"):
                assert np.array_equal(got.ravel(), ids[tail]), (name, key, k)
            elif want.dtype == np.float32 and not exact:
                np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6, err_msg=f"{name}:{key}@{k}")
            else:
                assert got.dtype == want.dtype and np.array_equal(got, want.reshape(got.shape)), (name, key, k)
        assert np.array_equal(a["info:env_id"].ravel(), ids)
        ends += int(a["done"].reshape(-1)[TRIP:].sum())
        if k == 12:
            break
        act = sample_actions(c, rng, BIG_N)
        big.send(ids, act)
        a, o = big.recv_dict(), orc.step(act[tail])
    if name == "Catch-v0":
        assert ends == 70  # every env of the second trip has ended its first episode and begun the next
    big.close()
    print(f"{name} N={BIG_N}: {time.time() - t0:.1f} s")


# ---- planar_lpt -----------------------------------------------------------------------------------
# The lane-group launcher files its chunks for longest-first dispatch only when chunks queue for waves:
# nchunks > resident (LaunchKl, mujoco_planar_lg.hip).  With "planar_layout" = 4 and one wave per SIMD, resident is the
# number of SIMDs -- 256 CUs x 4 = 1024 -- and a full chunk holds 64 / 4 = 16 envs; `per` reaches 16 from 12289 rows
# on, so nchunks = ceil(N / 16) first exceeds 1024 at N = 16 x 1024 + 1.  (The default layout turns to 2 lanes per env
# above 16384 rows, where the same arithmetic gives 32 x 1024 + 1: the key is set so that the smaller pool will do.)
LPT_N = 16 * 1024 + 1


@pytest.mark.parametrize("task", ["HalfCheetah-v4", "Walker2d-v4"])
def test_longest_first_dispatch_steps_alike(task):
    """"planar_lpt" 0 against 1: the order in which chunks are served comes from the previous whole-pool launch, so
    the run is 4 whole-pool steps, a send of 517 ids out of order (which breaks the chain), and 5 more whole-pool
    steps; episodes of 4 steps put resets on both sides of it."""
    pools = [Handle(task, seed=17, n=LPT_N, engine_keys={"planar_lpt": v, "planar_layout": 4}, max_episode_steps=4)
             for v in (0, 1)]
    rng = np.random.default_rng(7)
    rows = [h.reset() for h in pools]
    same_rows([rows[1]], [rows[0]], (task, "reset"))
    part = rng.permutation(LPT_N)[:517].astype(np.int32)
    resets = 0
    for t in range(10):
        ids = part if t == 4 else None
        act = pools[0].actions(rng, 517 if t == 4 else None)
        rows = [h.step(act, ids) for h in pools]
        same_rows([rows[1]], [rows[0]], (task, t))
        resets += int((rows[0]["elapsed_step"] == 0).sum())
    assert resets >= LPT_N
    for h in pools:
        h.close()


# ---- copy_threads, numa_bind ------------------------------------------------------------------
HOST_N = 32768 + 40  # HalfCheetah: its rows make more than the 4 MB from which a step is pipelined


@pytest.mark.parametrize("path", [{"step_pipeline": 16384, "direct_out": 0}, {"step_pipeline": 0, "direct_out": 2}],
                         ids=["pipelined", "direct_out=2"])
def test_host_copy_helpers_step_alike(path):
    """"copy_threads" 0 / 1 / 8 x "numa_bind" 0 / 1 on the two host steps whose action rows the helper threads stage
    -- the two-launch pipeline and the direct step that reads the actions in place -- against a pool with the default
    keys: 8 whole-pool steps of episodes of 3 steps."""
    from envpool_amd.core.device_pool import DevicePool

    combos = [{"copy_threads": c, "numa_bind": b} for c in (0, 1, 8) for b in (0, 1)]
    pools = [DevicePool("HalfCheetah", HOST_N, seed=19, max_episode_steps=3)]
    pools += [DevicePool("HalfCheetah", HOST_N, seed=19, max_episode_steps=3, params={**path, **c}) for c in combos]
    ids = np.arange(HOST_N, dtype=np.int32)
    rng = np.random.default_rng(9)
    for p in pools:
        p.reset(ids)
    rows = [recv_rows(p) for p in pools]
    resets = 0
    for t in range(9):
        for c, r in zip(combos, rows[1:]):
            same_rows([r], [rows[0]], (path, c, t))
        if t == 8:
            break
        act = rng.uniform(-1, 1, (HOST_N, 6))
        for p in pools:
            p.send(ids, act)
        rows = [recv_rows(p) for p in pools]
        resets += int((rows[0]["elapsed_step"] == 0).sum())
    assert resets >= HOST_N
    for p in pools:
        p.close()
