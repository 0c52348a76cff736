"""PGX self-play recorder, CPU side: envpool_amd/csrc/pgx_record.hip.h built for the host by g++ (a harness that walks
the lanes as loops) against the contract restated in numpy (pgx_record_util.Model) and, without symmetries, against the
samples the reference's own fixtures hold; the symmetry tables against the game's own step; and the argument checks of
the Python wrappers, which come before any native call."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pgx_record_util as R
from pgx_util import ACTIONS, CODE, NAMES, fixture, game, hidden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMES = ["TicTacToe-v1", "ConnectFour-v1", "Hex-v1", "Othello-v1"]
DIMS = {"TicTacToe": (3, 3, 2), "ConnectFour": (6, 7, 2), "Hex": (11, 11, 4), "Othello": (8, 8, 2)}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pgx_record") / "libpgxrecordhost.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "cpu_harness", "pgx_record_host.cpp"), "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.pgx_record_begin.restype = ctypes.c_void_p
    for f in (L.pgx_record_counters, L.pgx_record_staged, L.pgx_record_drain, L.pgx_record_discard, L.pgx_record_end):
        f.restype = None
    return L


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Host:
    """The harness's recorder over the envs of fixture `name`."""

    def __init__(self, lib, name, n_envs, capacity, max_plies=0, symmetries=False, id_offset=0, block=1024):
        self.lib, self.name, self.gm, self.block = lib, name, game(name), block
        self.g, self.hid = fixture(name), np.ascontiguousarray(hidden(fixture(name)), np.int32)
        self.h = ctypes.c_void_p(lib.pgx_record_begin(CODE[self.gm], n_envs, capacity, max_plies, int(symmetries),
                                                      id_offset))

    def add_rows(self, ids, hid, over, elapsed, policy):
        ids = np.ascontiguousarray(ids, np.int32)
        args = [np.ascontiguousarray(hid, np.int32), np.ascontiguousarray(over, np.uint8),
                np.ascontiguousarray(elapsed, np.int32), R.bits(policy)]
        assert self.lib.pgx_record_add(self.h, len(ids), _ptr(ids), *[_ptr(a) for a in args]) == 0

    def add(self, t, ids, rows=None):
        """Stages fixture row t of the fixture envs `rows` (default: ids) as the recorder's envs `ids`."""
        rows = ids if rows is None else rows
        self.add_rows(ids, self.hid[t, rows], self.g["done"][t, rows], self.g["elapsed_step"][t, rows],
                      R.policy_rows(self.name, t, self.g["done"].shape[1])[rows])

    def finish(self, ids, reward, done):
        ids = np.ascontiguousarray(ids, np.int32)
        reward, done = R.bits(reward), np.ascontiguousarray(done, np.uint8)
        assert self.lib.pgx_record_finish(self.h, len(ids), _ptr(ids), _ptr(reward), _ptr(done), self.block) == 0

    def count(self):
        return self.lib.pgx_record_count(self.h)

    def counters(self):
        c = np.zeros(4, np.int64)
        self.lib.pgx_record_counters(self.h, _ptr(c))
        return dict(zip(("samples", "games", "dropped_games", "dropped_plies"), (int(x) for x in c)))

    def drain(self):
        n, a = self.count(), ACTIONS[self.gm]
        out = (np.zeros((n,) + DIMS[self.gm], np.uint8), np.zeros((n, a), np.uint8), np.zeros((n, a), np.uint32),
               np.zeros(n, np.uint32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint8))
        self.lib.pgx_record_drain(self.h, *[_ptr(o) for o in out])
        assert self.count() == 0
        return out

    def discard(self, ids):
        ids = np.ascontiguousarray(ids, np.int32)
        self.lib.pgx_record_discard(self.h, len(ids), _ptr(ids))

    def close(self):
        self.lib.pgx_record_end(self.h)


def model_add(model, name, t, ids, rows=None):
    """What Host.add stages, read off the fixture's observation rows for the restatement."""
    g = fixture(name)
    rows = ids if rows is None else rows
    cp = g["info:current_player"][t, rows]
    model.add(ids, g["done"][t, rows], g["elapsed_step"][t, rows], cp, g["obs"][t, rows, cp],
              g["info:legal_action_mask"][t, rows], R.policy_rows(name, t, g["done"].shape[1])[rows])


def both(lib, name, capacity, steps, **kw):
    """The harness and the restatement side by side through the first `steps` steps of a fixture."""
    g = fixture(name)
    n = g["done"].shape[1]
    ids = np.arange(n, dtype=np.int32)
    host, model = Host(lib, name, n, capacity, **kw), R.Model(game(name), n, capacity, **{
        k: v for k, v in kw.items() if k != "block"})
    for t in range(steps):
        host.add(t, ids)
        model_add(model, name, t, ids)
        host.finish(ids, g["reward"][t + 1], g["done"][t + 1])
        model.finish(ids, g["reward"][t + 1], g["done"][t + 1])
    return host, model


@pytest.mark.parametrize("name", NAMES)
def test_whole_fixture_against_the_restatement_and_the_fixture(lib, name):
    g = fixture(name)
    host, model = both(lib, name, 8192, len(g["actions"]), id_offset=5)
    want, (games, plies) = R.fixture_samples(name, id_offset=5)
    if name in R.GAMES:
        assert (games, plies) == R.GAMES[name]
    elif name in R.SCRIPTED_GAMES:
        assert (games, plies) == R.SCRIPTED_GAMES[name]
    else:
        assert games == R.TRUNC_GAMES[name]
    assert host.counters() == model.counters == dict(samples=plies, games=games, dropped_games=0, dropped_plies=0)
    assert host.count() == plies
    got = host.drain()
    R.assert_same(got, model.drain(), name)
    R.assert_same(got, want, name)
    # what the samples are made of: wins of both seats, draws (not in every game), and a cleaned policy
    if name in R.GAMES:
        assert set(np.unique(got[3].view(np.float32))) >= {-1.0, 1.0}
    assert np.isfinite(got[2].view(np.float32)).all() and not got[2][got[1] == 0].any()
    host.close()


@pytest.mark.parametrize("name", GAMES)
def test_symmetries_against_the_restatement(lib, name):
    # TicTacToe and ConnectFour whole, the first 200 steps of Hex and Othello
    steps = len(fixture(name)["actions"]) if game(name) in ("TicTacToe", "ConnectFour") else 200
    host, model = both(lib, name, 1 << 15, steps, symmetries=True, block=5)
    nsym = R.NSYM[game(name)]
    assert lib.pgx_record_syms(CODE[game(name)]) == nsym
    plain, _ = R.fixture_samples(name, steps=steps)
    assert host.count() == nsym * len(plain[0]) > 0
    got = host.drain()
    R.assert_same(got, model.drain(), name)
    # order (game, ply, j): the samples of symmetry 0 are the plain recorder's, and sym counts 0 .. nsym - 1
    assert np.array_equal(got[6], np.tile(np.arange(nsym, dtype=np.uint8), len(plain[0])))
    R.assert_same(tuple(x[::nsym] for x in got), plain, name)
    host.close()


@pytest.mark.parametrize("name", GAMES)
def test_every_symmetry_commutes_with_the_games_step(lib, name):
    """sigma_j(step(position, a)) == step(sigma_j(position), sigma_j(a)) for legal a: obs of both seats, mask, done and
    rewards -- on fixture positions as hidden words, with the header's cell and action tables (which are also held
    against numpy's own rot90 / transpose / flips)."""
    gm, code = game(name), CODE[game(name)]
    g, hid = fixture(name), np.ascontiguousarray(hidden(fixture(name)), np.int32)
    h, w, c = DIMS[gm]
    a_n, cells, nsym = ACTIONS[gm], h * w, R.NSYM[gm]
    for j in range(nsym):
        cell_to = np.array([lib.pgx_record_sym_cell(code, j, x, 0) for x in range(cells)])
        act_to = np.array([lib.pgx_record_sym_action(code, j, x, 0) for x in range(a_n)])
        assert sorted(cell_to) == list(range(cells)) and sorted(act_to) == list(range(a_n))
        assert all(lib.pgx_record_sym_cell(code, j, int(cell_to[x]), 1) == x for x in range(cells))
        assert all(lib.pgx_record_sym_action(code, j, int(act_to[x]), 1) == x for x in range(a_n))
        where = np.arange(cells).reshape(h, w)
        assert np.array_equal(R.sym_board(gm, j, where).reshape(-1)[cell_to], np.arange(cells))
        assert np.array_equal(R.sym_actions(gm, j, np.arange(a_n))[act_to], np.arange(a_n))

    def step(words, action):
        obs, mask = np.zeros((2, h, w, c), np.uint8), np.zeros(a_n, np.uint8)
        done, rew, out = ctypes.c_int32(-1), np.zeros(2, np.float32), np.zeros_like(words)
        assert lib.pgx_record_step(code, _ptr(words), int(action), _ptr(obs), _ptr(mask), ctypes.byref(done),
                                   _ptr(rew), _ptr(out)) == 0
        return obs, mask, done.value, rew

    rng = np.random.default_rng(11)
    live = np.argwhere(~g["done"][:-1])
    picked = live[rng.choice(len(live), size=min(len(live), 200), replace=False)]
    last = np.argwhere(~g["done"][:-1] & g["done"][1:])[:40]  # ... and positions whose fixture move ends the game
    picked = np.concatenate([picked, last])
    assert len(picked) >= 200 and len(last) > 0
    ended = 0
    for t, e in picked:
        words = hid[t, e].copy()
        legal = np.flatnonzero(g["info:legal_action_mask"][t, e])
        actions = {int(g["actions"][t, e]), int(legal[rng.integers(len(legal))])} & set(int(x) for x in legal)
        for act in actions:
            obs, mask, done, rew = step(words, act)
            ended += done
            for j in range(1, nsym):
                turned = words.copy()
                turned[:cells] = R.sym_board(gm, j, words[:cells].reshape(h, w)).reshape(-1)
                act_t = int(R.sym_actions(gm, j, np.arange(a_n) == act).argmax())
                assert act_t == lib.pgx_record_sym_action(code, j, act, 0)
                obs_t, mask_t, done_t, rew_t = step(turned, act_t)
                assert done_t == done and np.array_equal(rew_t, rew), (name, j, t, e, act)
                for seat in range(2):
                    assert np.array_equal(obs_t[seat], R.sym_board(gm, j, obs[seat])), (name, j, t, e, act, seat)
                assert np.array_equal(mask_t, R.sym_actions(gm, j, mask)), (name, j, t, e, act)
    assert ended > 0


def test_max_plies_truncates_games_and_counts_the_plies(lib):
    name = "ConnectFour-v1"
    host, model = both(lib, name, 8192, 300, max_plies=4)
    c = host.counters()
    assert c == model.counters and c["dropped_plies"] > 0 and c["dropped_games"] == 0
    got = host.drain()
    _, (games, plies) = R.fixture_samples(name, steps=300)
    # (a few games end earlier, by an illegal move; the plies beyond four of the others are counted, not staged)
    assert c["games"] == games and c["samples"] == len(got[0]) < 4 * games and got[4].max() == 3
    assert np.bincount(got[5]).max() > 4 and np.all(np.bincount(got[4]) <= games)
    assert c["samples"] + c["dropped_plies"] >= plies  # (>: plies of games still running at the end)
    R.assert_same(got, model.drain(), name)
    host.close()


def _stage_some(lib, name, n_envs, capacity, rounds, **kw):
    """Recorders whose envs e have staged min(e % 3 + 1, rounds) plies: fixture rows t = 0 .. of fixture env e % 8."""
    g = fixture(name)
    host, model = Host(lib, name, n_envs, capacity, **kw), R.Model(game(name), n_envs, capacity, **{
        k: v for k, v in kw.items() if k != "block"})
    for t in range(rounds):
        assert not g["done"][t].any()
        ids = np.array([e for e in range(n_envs) if e % 3 + 1 > t], np.int32)
        host.add(t, ids, ids % 8)
        model_add(model, name, t, ids, ids % 8)
    return host, model


@pytest.mark.parametrize("block", [1, 4, 1024])
def test_capacity_admits_the_first_games_of_a_finish_and_drops_the_rest_whole(lib, block):
    name = "TicTacToe-v1"
    n = 11  # staged plies 1 2 3 1 2 3 1 2 3 1 2
    rng = np.random.default_rng(3)
    reward = rng.choice(np.array([-1, 0, 1], np.float32), size=(n, 2))
    ids = np.arange(n, dtype=np.int32)
    done = np.ones(n, bool)
    done[4] = False
    # rows 0 .. 3 hold 1 + 2 + 3 + 1 = 7 samples, row 5 (3 plies) does not fit into 9, and so nothing behind it does
    host, model = _stage_some(lib, name, n, 9, 3, block=block)
    host.finish(ids, reward, done)
    model.finish(ids, reward, done)
    assert host.count() == 7
    assert host.counters() == model.counters == dict(samples=7, games=4, dropped_games=6,
                                                     dropped_plies=3 + 1 + 2 + 3 + 1 + 2)
    staged = np.full(n, -1, np.int32)
    lib.pgx_record_staged(host.h, _ptr(staged))
    assert staged.tolist() == [0, 0, 0, 0, 2] + [0] * 6  # dropped games are gone too; row 4 is untouched
    # the next finish goes on at the count: env 4's game of 2 fits exactly
    done[:] = True
    host.finish(ids, reward, done)
    model.finish(ids, reward, done)
    assert host.count() == 9 and host.counters() == model.counters
    got = host.drain()
    R.assert_same(got, model.drain(), name)
    assert got[5].tolist() == [0, 1, 1, 2, 2, 2, 3, 4, 4]
    host.close()


def test_an_abandoned_game_is_discarded_at_the_next_add(lib):
    name = "Othello-v1"
    n = 8
    ids = np.arange(n, dtype=np.int32)
    host, model = _stage_some(lib, name, n, 64, 3)
    # envs 2 and 5 (3 plies staged) are reset behind the recorder's back: elapsed step 0 again
    back = np.array([2, 5], np.int32)
    host.add(0, back)
    model_add(model, name, 0, back)
    assert host.counters() == model.counters == dict(samples=0, games=0, dropped_games=2, dropped_plies=6)
    # discard: env 1 forgets its plies without a count
    host.discard(np.array([1], np.int32))
    model.discard([1])
    reward = np.tile(np.array([1, -1], np.float32), (n, 1))
    host.finish(ids, reward, np.ones(n, bool))
    model.finish(ids, reward, np.ones(n, bool))
    got = host.drain()
    R.assert_same(got, model.drain(), name)
    assert np.bincount(got[5], minlength=n).tolist() == [1, 0, 1, 1, 2, 1, 1, 2]
    host.close()


def test_finish_follows_the_calls_row_order_with_permuted_and_partial_ids(lib):
    name = "ConnectFour-v1"
    n = 9
    host, model = _stage_some(lib, name, n, 64, 3, symmetries=True)
    ids = np.array([7, 2, 8, 0, 5], np.int32)
    reward = np.arange(10, dtype=np.float32).reshape(5, 2)
    done = np.array([1, 1, 0, 1, 1], bool)
    host.finish(ids, reward, done)
    model.finish(ids, reward, done)
    got = host.drain()
    R.assert_same(got, model.drain(), name)
    assert got[5][::2].tolist() == [7, 7, 2, 2, 2, 0, 5, 5, 5]
    # the value is the mover's entry of the row's reward pair
    assert set(got[3].view(np.float32)[:4]) <= {0.0, 1.0}
    # the others are still staged
    rest = np.array([1, 3, 4, 6, 8], np.int32)
    host.finish(rest, np.zeros((5, 2), np.float32), np.ones(5, bool))
    model.finish(rest, np.zeros((5, 2), np.float32), np.ones(5, bool))
    R.assert_same(host.drain(), model.drain(), name)
    host.close()


def test_argument_refusals_come_before_any_native_call():
    from envpool_amd.core import native
    from envpool_amd.core.device_pool import DevicePool

    for bad in (0, -1, 2**31, 1.5, True):
        with pytest.raises(ValueError, match="recorder: capacity"):
            native.check_record(bad, 0, False)
    for bad in (-1, 257, 2.5, True):
        with pytest.raises(ValueError, match="recorder: max_plies"):
            native.check_record(16, bad, False)
    with pytest.raises(ValueError, match="recorder: symmetries"):
        native.check_record(16, 0, 1)
    assert native.check_record(16, 0, np.bool_(True)) == (16, 0, True)
    with pytest.raises(ValueError, match="must not be empty"):
        native.check_record_ids("recorder add", [])
    with pytest.raises(ValueError, match="recorder finish: env_ids must not repeat"):
        native.check_record_ids("recorder finish", [3, 1, 3])
    with pytest.raises(ValueError, match="recorder add: policy of shape"):
        native.check_record_add(np.zeros((2, 8)), 2, 9)
    with pytest.raises(ValueError, match="recorder finish: reward of shape"):
        native.check_record_finish(np.zeros((3, 2)), np.zeros(2, bool), 2)
    with pytest.raises(ValueError, match="recorder finish: done of shape"):
        native.check_record_finish(np.zeros((2, 2)), np.zeros(3, bool), 2)
    rew, done = native.check_record_finish(np.arange(4.0), np.array([0, 2]), 2)
    assert rew.shape == (2, 2) and rew.dtype == np.float32 and done.tolist() == [0, 1] and done.dtype == np.uint8
    # a pool without a native handle is never reached: the checks raise first
    pool = object.__new__(DevicePool)
    pool._lib = pool._h = None
    with pytest.raises(ValueError, match="recorder: capacity"):
        pool.record_begin(0)
    with pytest.raises(ValueError, match="recorder: max_plies"):
        pool.record_begin(8, 300)


def test_the_c_abi_states_the_headers_limits():
    from envpool_amd.core import native

    header = open(os.path.join(ROOT, "include", "envpool_amd.h")).read()
    for name in ("begin", "shape", "add", "add_device", "finish", "finish_device", "drain", "view_device", "clear",
                 "discard", "counters", "end"):
        assert f"epa_record_{name}" in native.EXPORTED_SYMBOLS and f"int epa_record_{name}(" in header
    assert "#define EPA_RECORD_MAX_PLIES 256" in header and native.RECORD_MAX_PLIES == 256
    assert "#define EPA_RECORD_SYMMETRIES 1u" in header and native.RECORD_SYMMETRIES == 1
    source = open(os.path.join(ROOT, "envpool_amd", "csrc", "pgx_record.hip.h")).read()
    assert "kRecordMaxPlies = 256" in source and "kRecordDefaultPlies = 128" in source


def test_a_family_without_a_recorder_raises():
    """HasRecord is false for every family but PGX (the engine's side is in test_gpu_pgx_record.py); here the Python
    side without a device: a pool with its own executor has no `record_begin` at all."""
    from envpool_amd.classic_control import CartPoleGymnasiumEnvPool

    env = object.__new__(CartPoleGymnasiumEnvPool)
    env._pool = object()
    with pytest.raises(RuntimeError, match="recorder not implemented for this environment"):
        env.recorder(16)
    with pytest.raises(ValueError, match="recorder: capacity"):
        env.recorder(0)
