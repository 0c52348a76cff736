"""PGX self-play recorder on the MI355X: the reference's fixtures replayed through DevicePool with `record_add` before
every step and `record_finish` after it, the drained samples bit for bit against the contract restated in numpy
(pgx_record_util.Model, fed with what the pool's recv returned) and against the rows of the fixture itself; the board
symmetries; the edges of the one-block scan; overflow, discard, a forced reset and an open guided session; the device
forms; a sharded pool."""
import numpy as np
import pytest

import envpool_amd as envpool
import pgx_record_util as R
from envpool_amd.core.device_pool import DevicePool
from pgx_util import ACTIONS, fixture, game

pytestmark = pytest.mark.gpu

ONE_EACH = ["TicTacToe-v1", "ConnectFour-v1", "Hex-v1", "Othello-v1"]
NAMES = ("samples", "games", "dropped_games", "dropped_plies")


def counters(pool):
    return dict(zip(NAMES, (int(x) for x in pool.record_counters()[1:])))


def rows_of(rd, n):
    """What the restatement's add takes, read off a recv of all n envs in id order."""
    cp = rd["info:current_player"]
    obs = rd["obs"].reshape((n, 2) + rd["obs"].shape[1:])[np.arange(n), cp]
    return rd["done"], rd["elapsed_step"], cp, obs, rd["info:legal_action_mask"]


def replay(name, pool, model, steps, add=None, finish=None):
    """Fixture `name` through the pool's recorder and the restatement, all envs in id order at every step."""
    g = fixture(name)
    n = g["actions"].shape[1]
    ids = np.arange(n, dtype=np.int32)
    add = add or (lambda pol: pool.record_add(pol))
    finish = finish or (lambda rd: pool.record_finish(rd["reward"], rd["done"]))
    pool.reset(ids)
    rd = pool.recv_dict()
    for t in range(steps):
        pol = R.policy_rows(name, t, n)
        add(pol)
        model.add(ids, *rows_of(rd, n), pol)
        pool.send(ids, g["actions"][t])
        rd = pool.recv_dict()
        finish(rd)
        model.finish(ids, rd["reward"], rd["done"])


def fixture_pool(name, **kw):
    g = fixture(name)
    return DevicePool(game(name), g["actions"].shape[1], seed=int(g["seed"]),
                      max_episode_steps=int(g["max_episode_steps"]), **kw)


@pytest.mark.parametrize("name", ONE_EACH + ["ConnectFour-v1__trunc"])
def test_fixture_replay_gives_the_fixtures_samples(name):
    g = fixture(name)
    pool = fixture_pool(name, env_id_offset=3)
    ids = np.arange(3, 3 + g["actions"].shape[1], dtype=np.int32)
    assert pool.record_begin(8192) == R.stack([], game(name))[0].shape[1:] + (ACTIONS[game(name)], 1)
    model = R.Model(game(name), len(ids), 8192, id_offset=3)
    steps = len(g["actions"])
    n = len(ids)
    pool.reset(ids)
    rd = pool.recv_dict()
    for t in range(steps):
        pol = R.policy_rows(name, t, n)
        pool.record_add(pol, ids)
        model.add(ids - 3, *rows_of(rd, n), pol)
        pool.send(ids, g["actions"][t])
        rd = pool.recv_dict()
        pool.record_finish(rd["reward"], rd["done"], ids)
        model.finish(ids - 3, rd["reward"], rd["done"])
    want, (games, plies) = R.fixture_samples(name, id_offset=3)
    assert counters(pool) == model.counters == dict(samples=plies, games=games, dropped_games=0, dropped_plies=0)
    assert int(pool.record_counters()[0]) == plies > 0
    got = pool.record_drain()
    assert got[0].dtype == np.bool_ and got[2].dtype == np.float32 and got[6].dtype == np.uint8
    R.assert_same(got, model.drain(), name)
    R.assert_same(got, want, name)
    assert int(pool.record_counters()[0]) == 0 and len(pool.record_drain()[0]) == 0
    pool.record_end()
    with pytest.raises(ValueError, match="the pool has no recorder"):
        pool.record_drain()
    pool.close()


def turned_state(gm, j, st):
    """A get_state row [cur_step, done, board words, ...] with its board under sigma_j."""
    h, w = {"TicTacToe": (3, 3), "ConnectFour": (6, 7), "Hex": (11, 11), "Othello": (8, 8)}[gm]
    out = st.copy()
    out[2:2 + h * w] = R.sym_board(gm, j, st[2:2 + h * w].reshape(h, w)).reshape(-1)
    return out


@pytest.mark.parametrize("name", ONE_EACH)
def test_symmetries(name):
    gm = game(name)
    g = fixture(name)
    nsym = R.NSYM[gm]
    steps = len(g["actions"]) if gm in ("TicTacToe", "ConnectFour") else 200
    n = g["actions"].shape[1]
    pool = fixture_pool(name)
    assert pool.record_begin(1 << 15, symmetries=True)[4] == nsym
    model = R.Model(gm, n, 1 << 15, symmetries=True)
    replay(name, pool, model, steps)
    plain, (games, plies) = R.fixture_samples(name, steps=steps)
    assert counters(pool) == model.counters == dict(samples=plies * nsym, games=games, dropped_games=0,
                                                    dropped_plies=0)
    got = pool.record_drain()
    R.assert_same(got, model.drain(), name)
    assert np.array_equal(got[6], np.tile(np.arange(nsym, dtype=np.uint8), plies))  # order: (row, ply, j)
    R.assert_same(tuple(x[::nsym] for x in got), plain, name)
    # equivariance through the engine's own observation: a second pool whose env j is set to sigma_j of a position of
    # the first; sample j of env 0 is then sample 0 of env j
    st = pool.get_state()
    e = int(np.flatnonzero(st[:, 1] == 0)[0])
    second = DevicePool(gm, nsym, seed=1)
    second.reset(np.arange(nsym, dtype=np.int32))
    second.recv()
    second.set_state(np.stack([turned_state(gm, j, st[e]) for j in range(nsym)]))
    second.record_begin(256, symmetries=True)
    p = R.policy_rows(name, 999, 1)[0]
    second.record_add(np.stack([R.sym_actions(gm, j, p) for j in range(nsym)]))
    second.record_finish(np.tile(np.array([1, -1], np.float32), (nsym, 1)), np.ones(nsym, bool))
    s = R.as_bits(second.record_drain())
    assert len(s[0]) == nsym * nsym and s[5].tolist() == sorted(list(range(nsym)) * nsym) and s[1][0].any()
    for j in range(nsym):
        for x in s[:4]:
            assert np.array_equal(x[j], x[j * nsym]), (name, j)
    second.close()
    pool.close()


WIN_5 = [0, 3, 1, 4, 2]     # TicTacToe: the first mover fills the top row, 5 plies
WIN_6 = [0, 3, 1, 4, 8, 5]  # ... the second mover fills the middle row, 6 plies


def scripted(pool, model, n, steps, order, finish_ids=None):
    """TicTacToe: env e plays WIN_5 (e % 3 != 0) or WIN_6 over and over, so games end a ply apart; `order`: the id
    list of every add and finish."""
    ids = np.arange(n, dtype=np.int32)
    long = ids % 3 == 0
    clock = np.zeros(n, int)
    pool.reset(ids)
    rd = pool.recv_dict()
    for t in range(steps):
        rng = np.random.default_rng(t)
        pol = np.tile(rng.random((1, 9)).astype(np.float32), (n, 1)) + (ids % 7)[:, None].astype(np.float32)
        pool.record_add(pol[order], order)
        rows = rows_of(rd, n)
        model.add(order, *[r[order] for r in rows], pol[order])
        over = rd["done"]
        act = np.where(long, np.array(WIN_6)[clock % 6], np.array(WIN_5)[clock % 5]).astype(np.int32)
        clock = np.where(over, 0, clock + 1)  # (an env that is over resets on this step and ignores its action)
        pool.send(ids, act)
        rd = pool.recv_dict()
        fin = order if finish_ids is None else finish_ids
        rew = rd["reward"].reshape(n, 2)
        pool.record_finish(rew[fin], rd["done"][fin], fin)
        model.finish(fin, rew[fin], rd["done"][fin])


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_scan_edges(n):
    """The one-block scan of finish: pools around its trip size, all rows in id order and in reverse."""
    for reverse in (False, True):
        pool = DevicePool("TicTacToe", n, seed=5)
        pool.record_begin(16 * n)
        model = R.Model("TicTacToe", n, 16 * n)
        order = np.arange(n, dtype=np.int32)[::-1].copy() if reverse else np.arange(n, dtype=np.int32)
        scripted(pool, model, n, 8, order)
        assert counters(pool) == model.counters and model.counters["games"] == n
        assert model.counters["samples"] == 5 * n + (n + 2) // 3
        R.assert_same(pool.record_drain(), model.drain(), (n, reverse))
        pool.close()


def test_overflow_discard_forced_reset_and_an_open_guided_session():
    n = 96
    ids = np.arange(n, dtype=np.int32)
    # the 64 short games end together with 5 plies each: a capacity of 300 admits the first of them only, and the 32
    # long games, which end a step later, find the buffer full.  max_plies = 5: their sixth ply is not staged
    pool = DevicePool("TicTacToe", n, seed=5)
    plain = DevicePool("TicTacToe", n, seed=5)  # the same positions without a recorder: its guided session is the yardstick
    pool.record_begin(300, max_plies=5)
    model = R.Model("TicTacToe", n, 300, max_plies=5)
    for p in (pool, plain):
        p.reset(ids)
    rd = pool.recv_dict()
    plain.recv()
    roots = np.array([1, 2, 5, 64], np.int32)
    clock = 0
    results = []
    for t in range(7):
        pol = np.random.default_rng(t).random((n, 9)).astype(np.float32)
        if t == 2:  # the sessions open mid-game, and advance between add and finish from here on
            leaves = [p.guided_begin(roots, 4, 1.25) for p in (pool, plain)]
            assert all(np.array_equal(a, b) for a, b in zip(*leaves))
        pool.record_add(pol)
        model.add(ids, *rows_of(rd, n), pol)
        if 2 <= t < 7:
            pri = np.full((4, 9), 1 / 9, np.float32)
            leaves = [p.guided_advance(pri, np.zeros(4, np.float32)) for p in (pool, plain)]
            assert all(np.array_equal(a, b) for a, b in zip(*leaves))
        if t == 3:  # env 7 is reset behind the recorder's back, env 8's plies are discarded
            pool.reset(np.array([7], np.int32))
            pool.recv()
            pool.record_discard(np.array([8], np.int32))
            model.discard([8])
        act = np.where(ids % 3 == 0, WIN_6[clock % 6], WIN_5[clock % 5]).astype(np.int32)
        clock += 1
        for p in (pool, plain):
            p.send(ids, act)
        rd = pool.recv_dict()
        plain.recv()
        pool.record_finish(rd["reward"], rd["done"])
        model.finish(ids, rd["reward"], rd["done"])
    results = [p.guided_result() for p in (pool, plain)]
    assert all(np.array_equal(a, b) for a, b in zip(*results)) and results[0][0].sum() == 4 * 4
    c = counters(pool)
    assert c == model.counters
    assert c["dropped_games"] > 32 and c["dropped_plies"] > 5 * c["dropped_games"] and 295 < c["samples"] <= 300
    got = pool.record_drain()
    R.assert_same(got, model.drain(), "overflow")
    assert got[4].max() == 4 and 7 not in got[5] and np.count_nonzero(got[5] == 8) == 1
    pool.guided_end()
    plain.close()
    pool.close()


@pytest.mark.parametrize("name", ["ConnectFour-v1", "Othello-v1"])
def test_device_forms_equal_the_host_forms(name):
    import torch

    from envpool_amd import torch_interop as ti

    gm, g = game(name), fixture(name)
    n = g["actions"].shape[1]
    steps = min(len(g["actions"]), 150)
    dev = torch.device("cuda", 0)
    host = fixture_pool(name)
    host.record_begin(4096, symmetries=True)
    model = R.Model(gm, n, 4096, symmetries=True)
    replay(name, host, model, steps)
    want = host.record_drain()
    pool = fixture_pool(name)
    pool.record_begin(4096, symmetries=True)
    replay(name, pool, R.Model(gm, n, 4096, symmetries=True), steps,
           add=lambda pol: ti.recorder_add_device(pool, torch.from_numpy(pol).to(dev)),
           finish=lambda rd: ti.recorder_finish_device(pool, torch.from_numpy(rd["reward"]).to(dev),
                                                       torch.from_numpy(rd["done"]).to(dev)))
    arrays, count = ti.recorder_view_device(pool)
    k = int(count.cpu()[0])
    assert k == len(want[0]) > 0 and count.dtype == torch.int32 and arrays[0].shape[0] == 4096
    for a, b in zip(arrays, want):
        got = a[:k].cpu().numpy()
        assert got.dtype == b.dtype and got.tobytes() == b.tobytes()
    assert counters(pool) == counters(host)
    ti.recorder_clear(pool)
    assert int(count.cpu()[0]) == 0 and int(pool.record_counters()[0]) == 0
    R.assert_same(want, model.drain(), name)
    host.close()
    pool.close()


def test_sharded_pool_equals_the_unsharded():
    name = "Othello-v1"
    g = fixture(name)
    n = g["actions"].shape[1]
    out = []
    for device in ([0, 0], 0):
        env = envpool.make(name, "gymnasium", num_envs=n, device=device, seed=int(g["seed"]))
        rec = env.recorder(capacity=1 << 14, symmetries=True)  # (nothing is dropped: a shard's recorder has it all)
        assert rec.symmetries == 8 and len(rec) == 0
        env.reset()
        for t in range(150):
            rec.add(R.policy_rows(name, t, n))
            _, rew, term, trunc, _ = env.step(g["actions"][t])
            rec.finish(rew, term | trunc)
        n_samples = len(rec)
        s = rec.drain()
        assert s._fields == R.FIELDS and len(s.obs) == n_samples > 0 and len(rec) == 0
        out.append((s, rec.counters))
        rec.close()
        with pytest.raises(ValueError, match="recorder is closed"):
            rec.drain()
        env.close()
    assert out[0][1] == out[1][1]
    # the shards' samples come behind each other: the same samples, grouped by shard (envs 0 .. 3, then 4 .. 7)
    a, b = R.as_bits(out[0][0]), R.as_bits(out[1][0])
    order = np.argsort(b[5] >= n // 2, kind="stable")
    R.assert_same(a, tuple(x[order] for x in b), "sharded")
    plain, _ = R.fixture_samples(name, steps=150)
    R.assert_same(tuple(x[::8] for x in b), plain, "unsharded")


def test_refusals_and_other_families():
    pool = DevicePool("TicTacToe", 4, seed=1)
    with pytest.raises(ValueError, match="the pool has no recorder"):
        pool.record_counters()
    with pytest.raises(ValueError, match="above the limit of 2 GiB"):
        pool.record_begin(2**31 - 1)
    pool.record_begin(16)
    with pytest.raises(ValueError, match="out of range"):
        pool.record_add(np.zeros((1, 9), np.float32), [4])
    with pytest.raises(ValueError, match="must not repeat"):
        pool.record_add(np.zeros((2, 9), np.float32), [1, 1])
    pool.record_begin(8, symmetries=True)  # the next begin replaces the recorder
    assert pool.record_shape() == (3, 3, 2, 9, 8)
    pool.close()
    other = DevicePool("CartPole", 4, seed=1)
    with pytest.raises(RuntimeError, match="recorder not implemented for this environment"):
        other.record_begin(16)
    other.close()
