"""Shared helpers of the PGX board-game tests: the fixtures (tests/golden/make_pgx_golden.py), their ids, and the
comparison of what a pool returns with a fixture row."""
import functools
import glob
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REGISTRY = json.load(open(os.path.join(GOLDEN, "pgx_registry.json")))
SPECS = json.load(open(os.path.join(GOLDEN, "pgx_spec.json")))
IDS = sorted(REGISTRY)
NAMES = sorted(os.path.basename(p)[len("pgx_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "pgx_*.npz")))
GAME = {tid: REGISTRY[tid]["spec_cls"][:-len("EnvSpec")] for tid in IDS}
CODE = {"TicTacToe": 0, "ConnectFour": 1, "Hex": 2, "Othello": 3}  # epa::pgx::Game
ACTIONS = {"TicTacToe": 9, "ConnectFour": 7, "Hex": 122, "Othello": 65}
# every state key in the engine's order (the reference's StateSpec order)
KEYS = [k for k, _ in SPECS["TicTacToe-v1"]["state_spec"]]
PER_PLAYER = {k for k, s in SPECS["TicTacToe-v1"]["state_spec"] if s["shape"][:1] == [-1]}


@functools.lru_cache(maxsize=None)
def _load(name):
    with np.load(os.path.join(GOLDEN, f"pgx_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def fixture(name):
    """The fixture's arrays (a fresh dict over cached arrays: do not modify them)."""
    return dict(_load(name))


def task_id(name):
    return name.split("__")[0]


def game(name):
    return GAME[task_id(name)]


def max_steps(name):
    return int(fixture(name)["max_episode_steps"])


def hidden(g):
    """The fixture's hidden words as the engine reports them: Hex's union-find labels by their sign (the engine
    keeps stone sets, not labels; every output depends on the sign only)."""
    h = g["hidden"].astype(np.int64)
    if h.shape[-1] == 123:  # Hex: board[121] step_count player_order[0]
        h = h.copy()
        h[..., :121] = np.sign(h[..., :121])
    return h


def check_rows(out, g, t, where, env_rows=slice(None), id_offset=0):
    """Every state key of a recv (per-player keys as [k * 2, ...] rows) against fixture row t (env rows
    `env_rows` of the fixture, in order; the pool's env ids are the fixture's + `id_offset`)."""
    for k in KEYS:
        want = g[k][t][env_rows]
        got = np.asarray(out[k])
        if k in ("info:env_id", "info:players.env_id"):
            got = got - id_offset
        if k in PER_PLAYER:
            assert got.shape[0] == 2 * want.shape[0], (where, k, got.shape)
        assert np.array_equal(got.reshape(want.shape), want), (where, t, k)
