"""The Jumanji board-puzzle ids of the reference's registry (envpool/jumanji/registration.py), with the same
`register` kwargs and `Jumanji/<id>` aliases (pinned by tests/golden/jumanji_registry.json).  The other
Jumanji ids (the routing, packing, scheduling, multi-agent and dataset-backed ones) are not registered."""
from envpool_amd.registration import register

_TASKS = (
    ("Game2048-v1", "Game2048", 1000),
    ("Maze-v0", "Maze", 100),
    ("Minesweeper-v0", "Minesweeper", 90),
    ("RubiksCube-partly-scrambled-v0", "RubiksCubePartlyScrambled", 20),
    ("RubiksCube-v0", "RubiksCube", 200),
    ("SlidingTilePuzzle-v0", "SlidingTilePuzzle", 500),
    ("Snake-v1", "Snake", 4000),
)

for _task_id, _prefix, _max_steps in _TASKS:
    register(task_id=_task_id, aliases=(f"Jumanji/{_task_id}",), import_path="envpool_amd.jumanji",
             spec_cls=f"{_prefix}EnvSpec", dm_cls=f"{_prefix}DMEnvPool", gymnasium_cls=f"{_prefix}GymnasiumEnvPool",
             max_episode_steps=_max_steps)
