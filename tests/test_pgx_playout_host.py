"""PGX playouts, CPU side: the playout of envpool_amd/csrc/pgx_playout.hip.h built for the host by g++ against the
pick rule restated in numpy (pgx_playout_util.py) and played through the reference-pinned `pgx_replay` of the PGX host harness, ply by
ply; the bit selection and the mixer on their own; and the argument checks of the Python wrappers, which come before
any native call."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from pgx_playout_util import M64, pick, sm, stream
from pgx_util import CODE, KEYS, fixture, game, hidden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMES = ["TicTacToe-v1", "ConnectFour-v1", "Hex-v1", "Othello-v1"]
SEED = 15  # covers a picked Hex swap and a picked Othello pass (test_seed_covers_the_swap_and_the_pass)
N_ENVS, REPEATS = 6, 3
ENV_IDS = np.array([3, 70000, 5, 11, 2**20 + 1, 0], np.int32)  # the global ids the streams are keyed by


# ---- the two harnesses ------------------------------------------------------------------------------------------
def _build(tmp, source, name):
    out = str(tmp / name)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "cpu_harness", source), "-o", out], check=True)
    return ctypes.CDLL(out)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pgx_playout")
    play = _build(tmp, "pgx_playout_host.cpp", "libpgxplayouthost.so")
    play.pgx_select_bit.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int]
    play.pgx_playout_mix.argtypes = [ctypes.c_uint64]
    play.pgx_playout_mix.restype = ctypes.c_uint64
    return _build(tmp, "pgx_host.cpp", "libpgxhost.so"), play


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def replay(lib, tid, seeds, acts):
    """pgx_replay of the columns `seeds` through the action rows `acts` [T, n]: {key: [T + 1, n, ...]}, hidden."""
    g = fixture(tid)
    acts = np.ascontiguousarray(acts, np.int32).reshape(-1, len(seeds))
    steps, n = acts.shape
    outs = {k: np.zeros((steps + 1, n) + g[k].shape[2:], g[k].dtype) for k in KEYS}
    code = CODE[game(tid)]
    hid = np.zeros((steps + 1, n, lib.pgx_hidden_words(code)), np.int32)
    ptrs = (ctypes.c_void_p * len(KEYS))(*[outs[k].ctypes.data for k in KEYS])
    seeds = np.ascontiguousarray(seeds, np.int32)
    assert lib.pgx_replay(code, n, steps, _ptr(seeds), _ptr(acts), 2**31 - 1, ptrs, _ptr(hid)) == 0
    return outs, hid


def start_row(tid, mid_game):
    """From reset: row 0.  Mid-game: the fixture's first ply row at which some of the envs are done and some not."""
    if not mid_game:
        return 0
    done = fixture(tid)["done"][:, :N_ENVS]
    return next(t for t in range(1, len(done)) if done[t].any() and not done[t].all())


def expected(lib, tid, t0, seed, max_plies):
    """Every (env, repeat) as its own replay column: the fixture's actions up to row t0, then the picks of the numpy
    rule from the masks the replay returns, the prefix replayed again for every ply.  Returns what a playout from row
    t0 has to report, the picked actions, and the hidden words and done flag it ends in."""
    g = fixture(tid)
    cols = [(i, r) for i in range(N_ENVS) for r in range(REPEATS)]
    seeds = np.array([int(g["seed"]) + i for i, _ in cols], np.int32)
    acts = [np.array([g["actions"][t, i] for i, _ in cols], np.int32) for t in range(t0)]
    hs = [stream(seed, ENV_IDS[i], r) for i, r in cols]
    limit = 256 if max_plies == 0 else max_plies
    plies = np.zeros(len(cols), np.int32)
    running = None
    picked = []
    while True:
        outs, hid = replay(lib, tid, seeds, np.array(acts, np.int32).reshape(len(acts), len(cols)))
        last = len(acts)
        if running is None:
            running = ~outs["done"][t0]
            end = np.full(len(cols), t0)
        else:
            running &= ~outs["done"][last]
        running &= plies < limit
        if not running.any():
            break
        row = np.zeros(len(cols), np.int32)
        for c in np.flatnonzero(running):
            row[c] = pick(outs["info:legal_action_mask"][last, c], hs[c], int(plies[c]))
            picked.append(int(row[c]))
            plies[c] += 1
            end[c] = last + 1
        acts.append(row)
    c = np.arange(len(cols))
    returns = np.array([outs["reward"][t0 + 1:end[j] + 1, j].sum(0) for j in c], np.float32)
    status = (~outs["done"][end, c]).astype(np.uint8)
    shape = (N_ENVS, REPEATS)
    return dict(returns=returns.reshape(*shape, 2), plies=plies.reshape(shape), status=status.reshape(shape),
                hidden=hid[end, c].reshape(*shape, -1), done=outs["done"][end, c].reshape(shape), picked=picked,
                start_hidden=hid[t0, ::REPEATS], start_done=outs["done"][t0, ::REPEATS])


def host_playout(play, tid, start_hidden, start_done, seed, max_plies):
    code = CODE[game(tid)]
    w = start_hidden.shape[1]
    hid = np.ascontiguousarray(start_hidden, np.int32)
    done = np.ascontiguousarray(start_done, np.uint8)
    returns = np.zeros((N_ENVS, REPEATS, 2), np.float32)
    plies = np.zeros((N_ENVS, REPEATS), np.int32)
    status = np.zeros((N_ENVS, REPEATS), np.uint8)
    hid_out = np.zeros((N_ENVS, REPEATS, w), np.int32)
    done_out = np.zeros((N_ENVS, REPEATS), np.uint8)
    rc = play.pgx_playout(code, N_ENVS, _ptr(hid), _ptr(done), _ptr(ENV_IDS), REPEATS, max_plies,
                          ctypes.c_uint64(seed), _ptr(returns), _ptr(plies), _ptr(status), _ptr(hid_out),
                          _ptr(done_out))
    assert rc == 0
    return dict(returns=returns, plies=plies, status=status, hidden=hid_out, done=done_out.astype(bool))


CASES = [(tid, mid, 0) for tid in GAMES for mid in (False, True)] + [(tid, False, 7) for tid in GAMES]
_expected = {}


def _case(lib, tid, mid, max_plies):
    key = (tid, mid, max_plies)
    if key not in _expected:
        _expected[key] = expected(lib, tid, start_row(tid, mid), SEED, max_plies)
    return _expected[key]


@pytest.mark.parametrize("tid,mid,max_plies", CASES)
def test_host_playout_equals_the_replayed_pick_rule(libs, tid, mid, max_plies):
    """Returns, plies, status and -- the commit form -- the position each playout ends in, all exactly."""
    host, play = libs
    want = _case(host, tid, mid, max_plies)
    if mid:
        assert want["start_done"].any() and not want["start_done"].all()
        assert np.array_equal(want["start_hidden"], hidden(fixture(tid))[start_row(tid, True), :N_ENVS])
        assert (want["plies"][want["start_done"]] == 0).all() and (want["plies"][~want["start_done"]] > 0).all()
    if max_plies:  # the cut: some playouts stop at it
        assert (want["status"] == 1).any() and want["plies"].max() == max_plies
        assert ((want["status"] == 1) <= (want["plies"] == max_plies)).all()
    else:
        assert (want["status"] == 0).all()
    got = host_playout(play, tid, want["start_hidden"], want["start_done"], SEED, max_plies)
    for k in ("returns", "plies", "status", "hidden", "done"):
        assert np.array_equal(got[k], want[k]), (tid, mid, max_plies, k)
    assert set(np.unique(want["returns"])) <= {-1.0, 0.0, 1.0}


def test_seed_covers_the_swap_and_the_pass(libs):
    host, _ = libs
    assert 121 in _case(host, "Hex-v1", False, 0)["picked"]
    assert 64 in _case(host, "Othello-v1", False, 0)["picked"]


def test_select_bit_and_mixer(libs):
    _, play = libs
    rng = np.random.default_rng(3)
    sets = [1, 1 << 127, (1 << 128) - 1, 1 << 63, 1 << 64, (1 << 64) | 1, ((1 << 122) - 1)]
    sets += [int.from_bytes(rng.bytes(16), "little") & int.from_bytes(rng.bytes(16), "little") for _ in range(200)]
    for m in sets:
        bits = [i for i in range(128) if (m >> i) & 1]
        for j in sorted({0, len(bits) // 2, len(bits) - 1} | set(range(min(len(bits), 5)))):
            if j < len(bits):
                assert play.pgx_select_bit(m & M64, m >> 64, j) == bits[j], (hex(m), j)
    # splitmix64's published first outputs from state 0
    assert play.pgx_playout_mix(0) == 0xE220A8397B1DCDAF == sm(0)
    for x in [1, M64, 0x9E3779B97F4A7C15, 1234567]:
        assert play.pgx_playout_mix(x) == sm(x)


# ---- wrapper checks without a native call -------------------------------------------------------------------------
class _Recorder:
    def __init__(self):
        self.calls = []

    def playout(self, env_ids, repeats, max_plies, seed, commit):
        self.calls.append((np.asarray(env_ids), repeats, max_plies, seed, commit))
        k = len(env_ids)
        return np.zeros((k, repeats, 2), np.float32), np.zeros((k, repeats), np.int32), np.zeros((k, repeats), np.uint8)


def test_wrapper_checks_come_before_the_native_call():
    from envpool_amd.pgx import OthelloGymnasiumEnvPool

    env = object.__new__(OthelloGymnasiumEnvPool)
    env._pool = _Recorder()
    ids = np.array([2, 0, 1], np.int32)
    out = env.playout(ids, repeats=2, max_plies=9, seed=5)
    assert out._fields == ("returns", "plies", "status")
    assert out.returns.shape == (3, 2, 2) and out.plies.shape == (3, 2) and out.status.dtype == np.uint8
    assert len(env._pool.calls) == 1
    assert np.array_equal(env._pool.calls[0][0], ids) and env._pool.calls[0][1:] == (2, 9, 5, False)
    env.playout(ids, commit=True)
    assert len(env._pool.calls) == 2 and env._pool.calls[1][4] is True
    for kw in (dict(repeats=0), dict(repeats=4097), dict(max_plies=-1), dict(max_plies=257),
               dict(repeats=2, commit=True)):
        with pytest.raises(ValueError, match="playout"):
            env.playout(ids, **kw)
    with pytest.raises(ValueError, match="repeat"):
        env.playout(np.array([1, 2, 1], np.int32), commit=True)
    with pytest.raises(ValueError, match="empty"):
        env.playout(np.zeros(0, np.int32))
    assert len(env._pool.calls) == 2
