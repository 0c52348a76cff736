"""The 30 classic MiniGrid navigation ids of the reference's registry, with the same `register` kwargs
(pinned by tests/golden/minigrid_registry.json).  BabyAI, the room-grid tasks, MultiRoom, Memory, WFC and the
random-mission tasks are not registered.

Table rows: (task id, env_name, max_episode_steps, task kwargs).  A random start is
agent_start_pos = (-1, -1), agent_start_dir = -1."""
from envpool_amd.registration import register

_RANDOM = {"agent_start_pos": (-1, -1), "agent_start_dir": -1}
_DISTSHIFT = {"width": 9, "height": 7, "agent_start_pos": (1, 1), "agent_start_dir": 0}

_TASKS = (
    [(f"MiniGrid-Empty-{s}x{s}-v0", "empty", 4 * s * s, {"size": s}) for s in (5, 6, 8, 16)]
    + [(f"MiniGrid-Empty-Random-{s}x{s}-v0", "empty", 4 * s * s, {"size": s, **_RANDOM}) for s in (5, 6)]
    + [(f"MiniGrid-DoorKey-{s}x{s}-v0", "doorkey", 10 * s * s, {"size": s}) for s in (5, 6, 8, 16)]
    + [(f"MiniGrid-DistShift{v}-v0", "distshift", 4 * 9 * 7, {**_DISTSHIFT, "strip2_row": row})
       for v, row in ((1, 2), (2, 5))]
    + [(f"MiniGrid-{kind}CrossingS{s}N{n}-v0", "crossing", 4 * s * s,
        {"size": s, "num_crossings": n, "obstacle_type": obstacle})
       for kind, obstacle in (("Lava", "lava"), ("Simple", "wall")) for s, n in ((9, 1), (9, 2), (9, 3), (11, 5))]
    + [(f"MiniGrid-LavaGapS{s}-v0", "lava_gap", 4 * s * s, {"size": s, "obstacle_type": "lava"}) for s in (5, 6, 7)]
    + [(f"MiniGrid-Dynamic-Obstacles-{'Random-' if rnd else ''}{s}x{s}-v0", "dynamic_obstacles", 4 * s * s,
        {"size": s, "n_obstacles": n, "action_max": 2, **(_RANDOM if rnd else {})})
       for s, n, rnd in ((5, 2, False), (5, 2, True), (6, 3, False), (6, 3, True), (8, 4, False), (16, 8, False))]
    + [("MiniGrid-FourRooms-v0", "four_rooms", 100, {})]
)

for _task_id, _env_name, _max_steps, _kw in _TASKS:
    register(task_id=_task_id, import_path="envpool_amd.minigrid", spec_cls="MiniGridEnvSpec",
             dm_cls="MiniGridDMEnvPool", gymnasium_cls="MiniGridGymnasiumEnvPool",
             max_episode_steps=_max_steps, env_name=_env_name, **_kw)
