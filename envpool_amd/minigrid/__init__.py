"""MiniGrid navigation envs (mirror of envpool/minigrid/__init__.py, the 30 classic navigation ids).

The spec table restates `MiniGridEnvFns::{DefaultConfig,StateSpec,ActionSpec}` (minigrid/minigrid.h:33-80):
the whole config key set with the reference's defaults, string and pair keys included.  The engine runs
env_name empty / doorkey / distshift / crossing / lava_gap / dynamic_obstacles / four_rooms
(csrc/minigrid.hip); any other env_name raises.

Within those, `make(id, size=..., agent_start_pos=..., ...)` takes every config the engine can run bit for bit
with the reference: grid sides 5..19 (dynamic_obstacles: up to 16), DistShift `width` / `height` / `strip2_row`
inside the walls, a fixed `agent_start_pos` inside the walls with `agent_start_dir` 0..3 or `(-1, -1)` for a
random start, `n_obstacles` 0..8 after the reference's clamp, any `max_episode_steps`.  Everything else raises
ValueError when the pool is constructed, before anything runs.  Two refusals are stricter than the reference:
crossing needs an odd `size` (the reference CHECK-fails) and `num_crossings` in 1..2 * ((size - 3) / 2): with
more crossings than rivers the reference pads the river list with entries that put lava on the top wall row,
and `num_crossings = 0`, which the reference does run (a grid without rivers), is refused as well.

Every rejection-sampling loop of a reset is bounded by the engine key `minigrid_max_tries` (default 2^20;
`DevicePool("MiniGrid", ..., params={"minigrid_max_tries": n})`).  A reset that runs out raises RuntimeError
from `recv` (on the device path: from a later recv or `synchronize()`), where the reference would throw in a
worker thread or spin.  The error is sticky: every later recv of that pool raises, and the pool has to be
recreated.
"""

from __future__ import annotations

import numpy as np

from envpool_amd.core.binding import FamilyDef, make_native_classes, spec
from envpool_amd.python.api import py_env

# env_name -> the engine's task code (csrc/minigrid_env.hip.h, mg::Task)
ENV_NAMES = {"empty": 0, "doorkey": 1, "distshift": 2, "crossing": 3, "lava_gap": 4,
             "dynamic_obstacles": 5, "four_rooms": 6}

_DEFAULT_CONFIG = [
    ("env_name", "empty"), ("size", 8), ("width", 9), ("height", 7), ("agent_start_pos", (1, 1)),
    ("agent_start_dir", 0), ("agent_view_size", 7), ("mission_bytes", 96), ("action_max", 6),
    ("num_crossings", 1), ("obstacle_type", "lava"), ("strip2_row", 2), ("n_obstacles", 4), ("num_objs", 3),
    ("random_length", False), ("room_size", 6), ("num_rows", 3), ("num_cols", 3), ("obj_type", "ball"),
    ("wfc_preset", "MazeSimple"), ("ensure_connected", True), ("min_num_rooms", 2), ("max_num_rooms", 6),
    ("max_room_size", 10), ("key_in_box", True), ("blocked", True), ("agent_room", (1, 1)),
    ("num_quarters", 4), ("num_rooms_visited", 25), ("num_dists", 18), ("locked_room_prob", 0.5),
    ("locations", True), ("unblocking", True), ("implicit_unlock", True),
    ("action_kinds", "goto,pickup,open,putnext"), ("instr_kinds", "action,and,seq"), ("doors_open", False),
    ("debug", False), ("select_by", ""), ("first_color", ""), ("second_color", ""), ("strict", False),
    ("num_doors", 2), ("objs_per_room", 4), ("start_carrying", False), ("distractors", False),
]


def _state_spec(c: dict) -> list:
    v = c["agent_view_size"]
    bound = max(c["size"], c["width"], c["height"], 25)
    return [
        ("obs:direction", spec(np.int32, [-1], (0, 3))),
        ("obs:image", spec(np.uint8, [v, v, 3], (0, 255))),
        ("obs:mission", spec(np.uint8, [c["mission_bytes"]], (0, 255))),
        ("info:agent_pos", spec(np.int32, [2], (0, bound))),
        ("info:mission_id", spec(np.int32, [-1], (-1, 1024))),
    ]


def _native_params(c: dict) -> dict:
    name = c["env_name"]
    if name not in ENV_NAMES:
        raise ValueError(f"MiniGrid env_name {name!r} is not available on the MI355X engine "
                         f"(only {sorted(ENV_NAMES)})")
    if c["obstacle_type"] not in ("lava", "wall"):
        raise ValueError(f"MiniGrid obstacle_type {c['obstacle_type']!r}: only 'lava' or 'wall'")
    sx, sy = c["agent_start_pos"]
    return {
        "env_name_code": ENV_NAMES[name], "size": c["size"], "width": c["width"], "height": c["height"],
        "start_x": sx, "start_y": sy, "start_dir": c["agent_start_dir"], "num_crossings": c["num_crossings"],
        "obstacle_wall": int(c["obstacle_type"] == "wall"), "strip2_row": c["strip2_row"],
        "n_obstacles": c["n_obstacles"],
    }


_MiniGrid = FamilyDef(
    name="MiniGrid", native="MiniGrid",
    default_config=_DEFAULT_CONFIG,
    state_spec=_state_spec,
    action_spec=lambda c: [("action", spec(np.int32, [-1], (0, c["action_max"])))],
    native_params=_native_params,
    unsupported={"agent_view_size": 7, "mission_bytes": 96},
)

_MiniGridEnvSpec, _MiniGridEnvPool = make_native_classes(_MiniGrid)
MiniGridEnvSpec, MiniGridDMEnvPool, MiniGridGymnasiumEnvPool = py_env(_MiniGridEnvSpec, _MiniGridEnvPool)


def decode_mission(mission: np.ndarray) -> str | np.ndarray:
    """Text of an `obs:mission` row: the bytes up to the first NUL (WriteMission zero-pads the row), as UTF-8.
    A batch of rows gives an object array with one string per row."""
    rows = np.asarray(mission, dtype=np.uint8)
    if rows.ndim == 1:
        return rows.tobytes().split(b"\0", 1)[0].decode("utf-8")
    flat = rows.reshape(-1, rows.shape[-1])
    texts = np.empty(flat.shape[0], dtype=object)
    for i, row in enumerate(flat):
        texts[i] = row.tobytes().split(b"\0", 1)[0].decode("utf-8")
    return texts.reshape(rows.shape[:-1])


for _cls in (MiniGridEnvSpec, MiniGridDMEnvPool, MiniGridGymnasiumEnvPool):
    _cls.decode_mission = staticmethod(decode_mission)

__all__ = ["MiniGridEnvSpec", "MiniGridDMEnvPool", "MiniGridGymnasiumEnvPool", "decode_mission"]
