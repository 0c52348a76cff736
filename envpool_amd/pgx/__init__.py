"""PGX two-player board games (mirror of envpool/pgx/__init__.py for TicTacToe, ConnectFour, Hex and Othello).

The spec tables restate each `XxxEnvFns::{DefaultConfig,StateSpec,ActionSpec}` of envpool/pgx/board_games.h: the
config key set with the reference's defaults (the common keys plus `task`), the state keys and the action spec.
The engine runs csrc/pgx.hip.

These are the engine's multi-player families: `max_num_players` must be 2 (the registry passes it).  Every env
writes two player rows, so `reward`, `discount`, `info:players.env_id`, `info:players.id` and `obs` come back with
2 rows per env, env-major (`info:players.env_id` = 0 0 1 1 ...), like the reference's; the other keys have one row
per env.  An action is one row per env.  Divergence: the reference routes action rows to envs by `players.env_id`;
here a send whose `players.env_id` differs from `env_id` raises ValueError.
"""

from __future__ import annotations

import numpy as np

from envpool_amd.core.binding import FamilyDef, make_native_classes, spec
from envpool_amd.python.api import py_env

PLAYERS = 2
INT_MIN, INT_MAX = -(2**31), 2**31 - 1

# task (the reference's DefaultConfig), board rows / columns, observation channels, actions
GAMES = {
    "TicTacToe": ("tic_tac_toe", 3, 3, 2, 9),
    "ConnectFour": ("connect_four", 6, 7, 2, 7),
    "Hex": ("hex", 11, 11, 4, 122),
    "Othello": ("othello", 8, 8, 2, 65),
}


def _state_spec(h: int, w: int, c: int, a: int):
    return lambda conf: [
        ("obs", spec(np.bool_, [-1, h, w, c])),
        ("info:board", spec(np.int32, [h, w])),
        ("info:current_player", spec(np.int32, [])),
        ("info:legal_action_mask", spec(np.bool_, [a])),
        ("info:players.id", spec(np.int32, [-1], (0, 1))),
    ]


def _action_spec(a: int):
    return lambda conf: [("action", spec(np.int32, [-1], (0, a - 1)))]


FAMILIES: dict[str, FamilyDef] = {}
__all__: list[str] = []
for _name, (_task, _h, _w, _c, _a) in GAMES.items():
    FAMILIES[_name] = FamilyDef(name=_name, native=_name, default_config=[("task", _task)],
                                state_spec=_state_spec(_h, _w, _c, _a), action_spec=_action_spec(_a),
                                players=PLAYERS)
    _spec_cls, _pool_cls = make_native_classes(FAMILIES[_name])
    _names = (f"{_name}EnvSpec", f"{_name}DMEnvPool", f"{_name}GymnasiumEnvPool")
    for _cls_name, _cls in zip(_names, py_env(_spec_cls, _pool_cls)):
        assert _cls.__name__ == _cls_name, (_cls.__name__, _cls_name)
        globals()[_cls_name] = _cls
        __all__.append(_cls_name)
