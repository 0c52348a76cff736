"""Jumanji board puzzles (mirror of envpool/jumanji/__init__.py for Game2048, Minesweeper, SlidingTilePuzzle,
RubiksCube, RubiksCubePartlyScrambled, Snake and Maze).

The spec tables restate each `XxxEnvFns::{DefaultConfig,StateSpec,ActionSpec}` of the reference
(envpool/jumanji/*_env.h): the config key set with the reference's defaults, the state keys and the action
spec.  The initial-state keys are parsed here on the host exactly as the reference's `Parse*` helpers parse
them (`engine_config`) and uploaded once per pool; the engine runs csrc/jumanji.hip.  The replay hooks
(`game2048_replay_boards`, `minesweeper_replay_*`: the reference's alignment hooks against the JAX implementation)
are kept in the key set with their defaults; a non-empty value raises ValueError.

Snake's fruit placement at reset is a rejection loop without a bound in the reference; here it is bounded by
the engine key `snake_max_tries` (default 2^20; `DevicePool("Snake", ..., params={"snake_max_tries": n})`).
A reset that runs out raises RuntimeError from `recv` (on the device path: from a later recv or
`synchronize()`).  The error is sticky: every later recv of that pool raises, and the pool has to be recreated.
"""

from __future__ import annotations

import re

import numpy as np

from envpool_amd.core.binding import FamilyDef, make_native_classes, spec
from envpool_amd.python.api import py_env

# puzzle codes of the engine (csrc/jumanji_env.hip.h, jm::Puzzle) and the native family of each prefix
PUZZLE = {"Game2048": 0, "Minesweeper": 1, "SlidingTilePuzzle": 2, "RubiksCube": 3, "RubiksCubePartlyScrambled": 3,
          "Snake": 4, "Maze": 5}
NATIVE = {"Game2048": "Game2048", "Minesweeper": "Minesweeper", "SlidingTilePuzzle": "SlidingTilePuzzle",
          "RubiksCube": "RubiksCube", "RubiksCubePartlyScrambled": "RubiksCube", "Snake": "Snake", "Maze": "Maze"}
# the puzzles' own episode limits (CurrentMaxEpisodeSteps is this + 1); Game2048 and Minesweeper have none
TIME_LIMIT = {"Game2048": 0, "Minesweeper": 0, "SlidingTilePuzzle": 500, "RubiksCube": 200,
              "RubiksCubePartlyScrambled": 20, "Snake": 4000, "Maze": 100}
INIT_WORDS = 100
INT_MAX, INT_MIN = 2**31 - 1, -(2**31)

_STOI = re.compile(r"[ \t\n\v\f\r]*([+-]?[0-9]+)")


def _stoi(token: str) -> int:
    """std::stoi: leading white space, an optional sign, digits; the rest of the token is ignored."""
    m = _STOI.match(token)
    if m is None:
        raise ValueError(f"stoi: no conversion of {token!r}")
    v = int(m.group(1))
    if not INT_MIN <= v <= INT_MAX:
        raise ValueError(f"stoi: {token!r} is out of range")
    return v


def _tokens(text: str, limit: int | None = None) -> list[str]:
    """The tokens `while (std::getline(stream, token, ',') && index < limit)` converts: a trailing ',' ends
    the stream without an empty token."""
    toks = text.split(",")
    if toks and toks[-1] == "":
        toks.pop()
    return toks if limit is None else toks[:limit]


def _position(text: str, default: tuple[int, int], hi: int) -> tuple[int, int]:
    """ParsePosition (snake_env.h, maze_env.h): the default for an empty text or one without ','; else the
    two numbers around the first ',', each clamped to [0, hi]."""
    if text == "" or "," not in text:
        return default
    sep = text.index(",")
    return (min(max(_stoi(text[:sep]), 0), hi), min(max(_stoi(text[sep + 1:]), 0), hi))


def engine_config(prefix: str, c: dict) -> tuple[list[int], list[int]]:
    """(the ints of jm::Cfg, the kInitWords ints of the pool's initial state) of a config, as the reference's
    constructors parse it.  Cfg: puzzle, time_limit, use_init, add_random_cell, num_scrambles, num_mines,
    pos[4], max_tries (the caller's)."""
    init = [0] * INIT_WORDS
    use_init, add_random, scrambles, mines, pos = 0, 1, 0, 10, [0, 0, 0, 0]
    if prefix == "Game2048":
        text = c["game2048_initial_board"]
        for i, t in enumerate(_tokens(text, 16)):
            init[i] = _stoi(t)
        use_init = int(text != "")
        add_random = int(bool(c["game2048_add_random_cell"]))
    elif prefix == "Minesweeper":
        locs = sorted({v for v in (_stoi(t) for t in _tokens(c["minesweeper_mine_locations"])) if 0 <= v < 100})
        for v in locs:
            init[v] = 1
        use_init = int(len(locs) > 0)
        mines = len(locs) if locs else 10
    elif prefix == "SlidingTilePuzzle":
        text = c["sliding_tile_initial_puzzle"]
        init[:25] = [i + 1 for i in range(24)] + [0]
        for i, t in enumerate(_tokens(text, 25)):
            init[i] = _stoi(t)
        use_init = int(text != "")
    elif prefix in ("RubiksCube", "RubiksCubePartlyScrambled"):
        text = c["rubiks_cube_initial_cube"]
        init[:54] = [i // 9 for i in range(54)]
        for i, t in enumerate(_tokens(text, 54)):
            init[i] = int(np.int32(_stoi(t)).astype(np.int8))  # static_cast<std::int8_t>
        use_init = int(text != "")
        scrambles = int(c["rubiks_cube_num_scrambles"])
    elif prefix == "Snake":
        pos = [*_position(c["snake_head_position"], (0, 0), 11), *_position(c["snake_fruit_position"], (0, 1), 11)]
        use_init = int(c["snake_head_position"] != "")
    elif prefix == "Maze":
        text = c["maze_walls"]
        for i, t in enumerate(_tokens(text, 100)):
            init[i] = int(_stoi(t) != 0)
        use_init = int(text != "")
        pos = [*_position(c["maze_agent_position"], (0, 0), 9), *_position(c["maze_target_position"], (9, 9), 9)]
    else:
        raise ValueError(f"unknown Jumanji puzzle {prefix!r}")
    cfg = [PUZZLE[prefix], TIME_LIMIT[prefix], use_init, add_random, scrambles, mines, *pos]
    return cfg, init


def _native_params(prefix: str):
    def params(c: dict) -> dict:
        cfg, init = engine_config(prefix, c)
        names = ["puzzle", "time_limit", "use_init", "add_random_cell", "num_scrambles", "num_mines",
                 "pos0", "pos1", "pos2", "pos3"]
        out = dict(zip(names, cfg))
        out.update({f"init{i}": v for i, v in enumerate(init) if v != 0})
        return out

    return params


def _int(shape, lo=None, hi=None):
    return spec(np.int32, shape, None if lo is None else (lo, hi))


def _bool(shape):
    return spec(np.bool_, shape, (False, True))


_FAMILIES = {
    "Game2048": (
        [("game2048_initial_board", ""), ("game2048_replay_boards", ""), ("game2048_add_random_cell", True)],
        lambda c: [("obs:board", _int([4, 4])), ("obs:action_mask", _bool([4])),
                   ("info:highest_tile", _int([], 1, 1 << 30))],
        lambda c: [("action", _int([-1], 0, 3))],
        {"game2048_replay_boards": ""},
    ),
    "Minesweeper": (
        [("minesweeper_mine_locations", ""), ("minesweeper_replay_boards", ""), ("minesweeper_replay_rewards", ""),
         ("minesweeper_replay_done", "")],
        lambda c: [("obs:board", _int([10, 10], -1, 8)), ("obs:action_mask", _bool([10, 10])),
                   ("obs:num_mines", _int([], 0, 99)), ("obs:step_count", _int([], 0, 90))],
        lambda c: [("action", _int([-1, 2], 0, 9))],
        {"minesweeper_replay_boards": "", "minesweeper_replay_rewards": "", "minesweeper_replay_done": ""},
    ),
    "SlidingTilePuzzle": (
        [("sliding_tile_initial_puzzle", "")],
        lambda c: [("obs:puzzle", _int([5, 5], 0, 24)), ("obs:empty_tile_position", _int([2], 0, 4)),
                   ("obs:action_mask", _bool([4])), ("obs:step_count", _int([], 0, 500)),
                   ("info:prop_correctly_placed", spec(np.float32, [], (0.0, 1.0)))],
        lambda c: [("action", _int([-1], 0, 3))],
        {},
    ),
    "Snake": (
        [("snake_head_position", ""), ("snake_fruit_position", "")],
        lambda c: [("obs:grid", spec(np.float32, [12, 12, 5], (0.0, 1.0))), ("obs:step_count", _int([], 0, 3999)),
                   ("obs:action_mask", _bool([4]))],
        lambda c: [("action", _int([-1], 0, 3))],
        {},
    ),
    "Maze": (
        [("maze_walls", ""), ("maze_agent_position", ""), ("maze_target_position", "")],
        lambda c: [("obs:agent_position.row", _int([], 0, 9)), ("obs:agent_position.col", _int([], 0, 9)),
                   ("obs:target_position.row", _int([], 0, 9)), ("obs:target_position.col", _int([], 0, 9)),
                   ("obs:walls", _bool([10, 10])), ("obs:step_count", _int([], 0, 100)),
                   ("obs:action_mask", _bool([4]))],
        lambda c: [("action", _int([-1], 0, 3))],
        {},
    ),
}
for _prefix, _limit, _scrambles in (("RubiksCube", 200, 100), ("RubiksCubePartlyScrambled", 20, 20)):
    _FAMILIES[_prefix] = (
        [("rubiks_cube_num_scrambles", _scrambles), ("rubiks_cube_initial_cube", "")],
        (lambda limit: lambda c: [("obs:cube", spec(np.int8, [6, 3, 3], (0, 5))),
                                  ("obs:step_count", _int([], 0, limit))])(_limit),
        lambda c: [("action", spec(np.int32, [-1, 3], elementwise=([0, 0, 0], [5, 0, 2])))],
        {},
    )

FAMILIES: dict[str, FamilyDef] = {}
__all__ = ["engine_config"]
for _prefix, (_config, _state, _action, _unsupported) in _FAMILIES.items():
    FAMILIES[_prefix] = FamilyDef(name=_prefix, native=NATIVE[_prefix], default_config=_config, state_spec=_state,
                                  action_spec=_action, native_params=_native_params(_prefix), unsupported=_unsupported)
    _spec_cls, _pool_cls = make_native_classes(FAMILIES[_prefix])
    _names = (f"{_prefix}EnvSpec", f"{_prefix}DMEnvPool", f"{_prefix}GymnasiumEnvPool")
    for _name, _cls in zip(_names, py_env(_spec_cls, _pool_cls)):
        assert _cls.__name__ == _name, (_cls.__name__, _name)
        globals()[_name] = _cls
        __all__.append(_name)
