"""Shared helpers of the render tests: the fixtures (tests/golden/make_render_golden.py), the ids and engine
families of the ten games, and the g++ host harness over the shared render headers."""
import ctypes
import functools
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# game -> (harness family, harness game code, task ids, default (width, height))
GAMES = {
    "Game2048": (0, 0, ["Game2048-v1"], (256, 256)),
    "Minesweeper": (0, 1, ["Minesweeper-v0"], (256, 256)),
    "SlidingTilePuzzle": (0, 2, ["SlidingTilePuzzle-v0"], (256, 256)),
    "RubiksCube": (0, 3, ["RubiksCube-v0", "RubiksCube-partly-scrambled-v0"], (256, 256)),
    "Snake": (0, 4, ["Snake-v1"], (256, 256)),
    "Maze": (0, 5, ["Maze-v0"], (256, 256)),
    "TicTacToe": (1, 0, ["TicTacToe-v1"], (192, 192)),
    "ConnectFour": (1, 1, ["ConnectFour-v1"], (280, 240)),
    "Hex": (1, 2, ["Hex-v1"], (352, 352)),
    "Othello": (1, 3, ["Othello-v1"], (256, 256)),
}
SIZES = [(0, 0), (61, 45), (16, 16), (7, 30), (1, 1)]


@functools.lru_cache(maxsize=None)
def _load(game):
    with np.load(os.path.join(GOLDEN, f"render_{game}.npz")) as z:
        return {k: z[k] for k in z.files}


def fixture(game):
    """The fixture's arrays (a fresh dict over cached arrays: do not modify them)."""
    return dict(_load(game))


def tags(game):
    return json.loads(str(fixture(game)["tags"]))


def build_harness(directory):
    out = os.path.join(str(directory), "librenderhost.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "cpu_harness", "render_host.cpp"), "-o", out], check=True)
    return ctypes.CDLL(out)


def host_size(lib, game, width, height):
    fam, code = GAMES[game][:2]
    w, h = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.render_size(fam, code, width, height, ctypes.byref(w), ctypes.byref(h)) == 0
    return w.value, h.value


def host_paint(lib, game, words, width, height, band=0):
    """The host harness's frame of one state (its hidden words) at a resolved size, painted in bands of `band`
    rows (0: the whole frame at once).  The buffer starts out as 0x5a: every byte has to be painted."""
    fam, code = GAMES[game][:2]
    words = np.ascontiguousarray(words, np.int32)
    rgb = np.full((height, width, 3), 0x5A, np.uint8)
    rc = lib.render_paint(fam, code, words.ctypes.data_as(ctypes.c_void_p), width, height, band,
                          rgb.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, (game, rc)
    return rgb


def state_rows(game, hidden):
    """set_state rows of fixture states: (elapsed step 0, not done) + the hidden words."""
    hidden = np.atleast_2d(hidden)
    return np.concatenate([np.zeros((hidden.shape[0], 2)), hidden.astype(np.float64)], axis=1)
