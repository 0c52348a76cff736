"""Board rendering on the MI355X: the render kernel's frames of the fixture states (set_state) at every fixture
size, byte for byte against what the reference's own Render painted (tests/golden/render_*.npz) -- through
DevicePool.render, torch_interop.render_device, make(..., "gymnasium") and make(..., "dm"); the env id forms; an
unaligned device buffer; rendering in the middle of an async roll-out, which must show the state and leave the
stepping alone; and the errors."""
import numpy as np
import pytest

import envpool_amd as envpool
from envpool_amd.core.device_pool import DevicePool
from render_util import GAMES, SIZES, build_harness, fixture, host_paint, state_rows

pytestmark = pytest.mark.gpu
N = 8


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("render"))


def _states(game, n=N):
    """n set_state rows cycling through the fixture's states, and the fixture state of each row."""
    g = fixture(game)
    which = np.arange(n) % len(g["hidden"])
    return g, which, state_rows(game, g["hidden"][which])


def _want(g, which, s, rows):
    return g[f"frame_{s}"][which[np.asarray(rows)]]


@pytest.mark.parametrize("game", sorted(GAMES))
def test_device_pool_render_matches_reference(game):
    g, which, rows = _states(game)
    pool = DevicePool(game, N)
    pool.set_state(rows)
    for s, (w, h) in enumerate(SIZES):
        assert pool.render_size(w, h) == tuple(g["resolved"][s])
        ids = np.arange(N, dtype=np.int32)
        got = pool.render(ids, w, h)
        assert got.dtype == np.uint8 and got.shape == _want(g, which, s, ids).shape
        assert np.array_equal(got, _want(g, which, s, ids)), (game, (w, h))
        # permuted with a duplicate, k = 5; k = 1; camera_id is ignored
        some = [6, 1, 6, 3, 0]
        assert np.array_equal(pool.render(some, w, h, camera_id=2), _want(g, which, s, some)), (game, (w, h))
        assert np.array_equal(pool.render([N - 1], w, h), _want(g, which, s, [N - 1])), (game, (w, h))
    pool.close()


@pytest.mark.parametrize("game", sorted(GAMES))
def test_render_device_matches_reference(game):
    torch = pytest.importorskip("torch")
    from envpool_amd.torch_interop import render_device

    g, which, rows = _states(game)
    pool = DevicePool(game, N)
    pool.set_state(rows)
    for s, (w, h) in enumerate(SIZES):
        ids = [5, 2, 2, 7, 0]
        t = render_device(pool, ids, w, h)
        assert t.dtype == torch.uint8 and t.is_cuda and t.device.index == pool.device
        assert np.array_equal(t.cpu().numpy(), _want(g, which, s, ids)), (game, (w, h))
        # a buffer that starts 1 byte into a larger allocation: the stores' unaligned head and tail
        rw, rh = g["resolved"][s]
        nbytes = len(ids) * int(rh) * int(rw) * 3
        big = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=t.device)
        out = render_device(pool, ids, w, h, out=big[1:1 + nbytes])
        assert out.data_ptr() == big.data_ptr() + 1
        host = big.cpu().numpy()
        assert np.array_equal(host[1:1 + nbytes].reshape(out.shape), _want(g, which, s, ids)), (game, (w, h))
        assert host[0] == 0xA5 and (host[1 + nbytes:] == 0xA5).all(), (game, (w, h))  # nothing beyond the frames
    pool.close()


@pytest.mark.parametrize("game", sorted(GAMES))
def test_make_gymnasium_render_matches_reference(game):
    g, which, rows = _states(game)
    for tid in GAMES[game][2]:
        for s, (w, h) in enumerate(SIZES):
            env = envpool.make(tid, "gymnasium", num_envs=N, render_mode="rgb_array", render_width=w,
                               render_height=h, render_env_id=3)
            env.device_pool.set_state(rows)
            ids = np.array([4, 0, 7, 4, 2], np.int32)
            assert np.array_equal(env.render(ids), _want(g, which, s, ids)), (tid, (w, h))
            assert np.array_equal(env.render(list(ids)), _want(g, which, s, ids)), (tid, (w, h))
            assert np.array_equal(env.render(6), _want(g, which, s, [6])), (tid, (w, h))
            assert np.array_equal(env.render(np.int32(6)), _want(g, which, s, [6])), (tid, (w, h))
            assert np.array_equal(env.render(), _want(g, which, s, [3])), (tid, (w, h))  # render_env_id
            assert np.array_equal(env.render(camera_id=1), _want(g, which, s, [3])), (tid, (w, h))
            env.close()


@pytest.mark.parametrize("game", sorted(GAMES))
def test_make_dm_render_matches_reference(game):
    g, which, rows = _states(game)
    env = envpool.make(GAMES[game][2][0], "dm", num_envs=N, render_mode="rgb_array")
    env.device_pool.set_state(rows)
    ids = [1, 5, 5]
    assert np.array_equal(env.render(ids), _want(g, which, 0, ids)), game
    env.close()


@pytest.mark.parametrize("game", ["Snake", "Hex"])
def test_env_id_offset_and_sharded_pools(game):
    g, which, rows = _states(game)
    pool = DevicePool(game, N, env_id_offset=100)
    pool.set_state(rows)
    ids = [107, 100, 103, 103, 101]
    local = [i - 100 for i in ids]
    assert np.array_equal(pool.render(ids, 61, 45), _want(g, which, 1, local))
    with pytest.raises(ValueError, match="env_id 7 out of range"):
        pool.render([7], 61, 45)
    pool.close()
    # device=[0, 0]: shard 0 owns envs 0..3, shard 1 envs 4..7; ids of both interleaved, one of them twice
    env = envpool.make(GAMES[game][2][0], "gymnasium", num_envs=N, device=[0, 0], render_mode="rgb_array",
                       render_width=61, render_height=45)
    for s, p in enumerate(env.device_pool.pools):
        p.set_state(rows[4 * s:4 * s + 4])
    ids = [5, 0, 6, 1, 5, 3, 4]
    assert np.array_equal(env.render(ids), _want(g, which, 1, ids))
    assert np.array_equal(env.render(), _want(g, which, 1, [0]))
    with pytest.raises(ValueError, match="env_id 8 out of range"):
        env.render([1, 8])
    with pytest.raises(ValueError, match="must not be empty"):
        env.render([])
    env.close()


# how many values an action component of the roll-out below takes (every one of them is on the board)
MOD = {"Game2048": 4, "Minesweeper": 10, "SlidingTilePuzzle": 4, "RubiksCube": 3, "Snake": 4, "Maze": 4}


def _action(pool, game, rng, out):
    """Seeded actions for the envs of a recv: a legal move where the game reports its legal action mask (PGX),
    else any on-board action (an invalid one changes nothing or ends the episode)."""
    mask = out.get("info:legal_action_mask")
    if mask is not None:
        return (mask * rng.random(mask.shape)).argmax(1).astype(pool.action_dtype)
    k = len(out["info:env_id"])
    return rng.integers(0, MOD[game], (k, *pool.action_shape)).astype(pool.action_dtype)


@pytest.mark.parametrize("game", sorted(GAMES))
def test_render_amid_an_async_rollout(harness, game):
    """batch_size < num_envs, 20 free-running steps, half of the envs sent and not received: render shows every
    env as get_state reports it at that point (repainted on the host), and the recvs that follow return what a
    twin pool that never rendered returns."""
    pools = [DevicePool(game, N, batch_size=4, seed=11) for _ in range(2)]
    ids_all = np.arange(N, dtype=np.int32)
    rng = np.random.default_rng(5)
    for p in pools:
        p.reset(ids_all)
    for t in range(20):
        outs = [p.recv_dict() for p in pools]
        assert np.array_equal(outs[0]["info:env_id"], outs[1]["info:env_id"])
        ids = outs[0]["info:env_id"]
        assert ids.shape == (4,)
        act = _action(pools[0], game, rng, outs[0])
        for p in pools:
            p.send(ids, act)
    frames = pools[0].render(ids_all)
    state = pools[0].get_state()
    w, h = pools[0].render_size()
    for e in range(N):
        want = host_paint(harness, game, state[e, 2:].astype(np.int32), w, h)
        assert np.array_equal(frames[e], want), (game, e)
    assert len({frames[e].tobytes() for e in range(N)}) > 1  # the envs have gone their own ways
    for t in range(20, 26):
        outs = [p.recv_dict() for p in pools]
        for k in outs[0]:
            assert np.array_equal(outs[0][k], outs[1][k]), (game, t, k)
        ids = outs[0]["info:env_id"]
        act = _action(pools[0], game, rng, outs[0])
        for p in pools:
            p.send(ids, act)
        pools[0].render(ids_all, 16, 16)
    assert np.array_equal(pools[0].get_state(), pools[1].get_state())
    for p in pools:
        p.close()


def test_a_finished_env_shows_its_terminal_state_until_its_next_step(harness):
    """An illegal TicTacToe move ends the game: the frame keeps the terminal board until the env's next step,
    which resets it."""
    pool = DevicePool("TicTacToe", 2)
    ids = np.arange(2, dtype=np.int32)
    pool.reset(ids)
    pool.recv()
    for a in ([4, 4], [0, 4]):  # env 1 plays the occupied centre: an illegal move, the game is over
        pool.send(ids, np.array(a, np.int32))
        out = pool.recv_dict()
    assert list(out["done"]) == [False, True]
    state = pool.get_state()
    frames = pool.render(ids)
    for e in range(2):
        assert np.array_equal(frames[e], host_paint(harness, "TicTacToe", state[e, 2:].astype(np.int32), 192, 192))
    # the terminal board: StepGame put the second mover's stone on the occupied centre before the move was refused
    assert (frames[1] == (230, 70, 70)).all(axis=-1).any() and not (frames[1] == (30, 30, 30)).all(axis=-1).any()
    pool.send(ids, np.array([1, 0], np.int32))  # env 1 resets: an empty board
    pool.recv()
    blank = host_paint(harness, "TicTacToe", np.array([-1] * 9 + [0, 0], np.int32), 192, 192)
    assert np.array_equal(pool.render([1])[0], blank)
    pool.close()


def test_errors():
    pool = DevicePool("Maze", 4)
    with pytest.raises(ValueError, match="render env_ids must not be empty"):
        pool.render([])
    with pytest.raises(ValueError, match="env_id 4 out of range"):
        pool.render([0, 4])
    with pytest.raises(ValueError, match="env_id -1 out of range"):
        pool.render([-1])
    with pytest.raises(ValueError):
        pool.render([0], 5000, 16)  # a side the kernel's row band cannot hold
    pool.close()
    for tid in ("CartPole-v1", "MiniGrid-Empty-5x5-v0"):
        env = envpool.make(tid, "gymnasium", num_envs=2, render_mode="rgb_array")
        with pytest.raises(RuntimeError, match="render not implemented for this environment"):
            env.render()
        with pytest.raises(RuntimeError, match="render not implemented for this environment"):
            env.render([0, 1])
        env.close()
    env = envpool.make("Maze-v0", "gymnasium", num_envs=2)
    with pytest.raises(RuntimeError, match="render_mode must be set"):
        env.render()
    env.close()


def test_human_mode_raises_the_reference_errors():
    env = envpool.make("Maze-v0", "gymnasium", num_envs=2, render_mode="human")
    with pytest.raises(ValueError, match="only supports a single env_id"):
        env.render([0, 1])
    try:
        import cv2  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match="requires opencv-python"):
            env.render()
    env.close()
