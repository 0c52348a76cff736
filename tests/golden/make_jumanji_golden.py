"""Generates the Jumanji board-puzzle fixtures from the reference itself.  Run on a machine that has the
reference tree (it is not on the GPU boxes):

    python tests/golden/make_jumanji_golden.py [/path/to/reference]

It compiles jumanji_golden_driver.cc, which includes the reference's own envpool/jumanji/*_env.h in place
inside its own AsyncEnvPool, with the absl stand-ins of oracle/ref_shims (read only), into a temporary
directory outside the repository.  Then it writes data only:

  tests/golden/jumanji_registry.json   the `register` kwargs of the 7 board-puzzle ids
  tests/golden/jumanji_spec.json       per id: DefaultConfig key set / defaults, state and action specs
  tests/golden/jumanji_<name>.npz      8 envs x max(300, max_episode_steps + 20) seeded actions (some out of
                                       the action bounds, to exercise the clamps; env 0 steered by the
                                       driver from its hidden state): every state key after the reset and
                                       after every step (rows in env id order), the hidden state of every
                                       env after each of them (`hidden`, int32 words, layout per puzzle in
                                       HIDDEN below), the actions sent, the seed and the config (`config`,
                                       JSON of the keys set on top of the id's defaults)

<name> is the id for its default config, and <id>__<variant> for a config with initial-state keys set.
Before writing anything it asserts coverage: an auto-reset in every fixture; Game2048 game over;
Minesweeper mine hit, win and invalid action; SlidingTilePuzzle and RubiksCube solved and time limit;
Snake fruit eaten, self-collision and wall; Maze target reached, time limit and a terminal reset.
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
N, MIN_STEPS = 8, 300
PREFIX = {"Game2048-v1": "Game2048", "Minesweeper-v0": "Minesweeper", "SlidingTilePuzzle-v0": "SlidingTilePuzzle",
          "RubiksCube-v0": "RubiksCube", "RubiksCube-partly-scrambled-v0": "RubiksCubePartlyScrambled",
          "Snake-v1": "Snake", "Maze-v0": "Maze"}
# int32 words of the driver's hidden state per env
HIDDEN = {"Game2048": "board[16]", "Minesweeper": "board[100] mines[100] num_mines step_count",
          "SlidingTilePuzzle": "puzzle[25] empty_row empty_col step_count",
          "RubiksCube": "cube[54] step_count", "RubiksCubePartlyScrambled": "cube[54] step_count",
          "Snake": "body[144] head_row head_col tail_row tail_col fruit_row fruit_col length step_count",
          "Maze": "walls[100] agent_row agent_col target_row target_col step_count"}
SOLVED_TILES = ",".join(str(i) for i in list(range(1, 24)) + [0, 24])  # one move (right) from solved
WALLS = ",".join("1" if (r % 3 == 1 and c != (r * 7) % 10) else "0" for r in range(10) for c in range(10))
# (fixture name, id, config keys on top of the id's defaults); the partly-scrambled cube's initial cube is
# filled in from the one-scramble fixture (a cube one move from solved)
FIXTURES = [(tid, tid, {}) for tid in PREFIX] + [
    ("Game2048-v1__board", "Game2048-v1", {"game2048_initial_board": "1,2,1,2,2,1,2,1,1,2,1,2,2,1,2,0"}),
    ("Game2048-v1__nomove", "Game2048-v1", {"game2048_initial_board": "1,2,1,2,2,1,2,1,1,2,1,2,2,1,2,1",
                                            "game2048_add_random_cell": "0"}),
    ("Game2048-v1__fixed", "Game2048-v1", {"game2048_initial_board": "0,0,17,0,0,0,0,0,3,3,0,0,0,0,0,1",
                                           "max_episode_steps": "40"}),
    ("Minesweeper-v0__mines", "Minesweeper-v0", {"minesweeper_mine_locations": "3,14,25,3,36,47,58,69,70,81,92,99,0,123"}),
    ("SlidingTilePuzzle-v0__puzzle", "SlidingTilePuzzle-v0", {"sliding_tile_initial_puzzle": SOLVED_TILES}),
    ("RubiksCube-v0__scramble1", "RubiksCube-v0", {"rubiks_cube_num_scrambles": "1"}),
    ("RubiksCube-partly-scrambled-v0__cube", "RubiksCube-partly-scrambled-v0", {"rubiks_cube_initial_cube": None}),
    ("Snake-v1__positions", "Snake-v1", {"snake_head_position": "5,5", "snake_fruit_position": "5,7"}),
    ("Maze-v0__walls", "Maze-v0", {"maze_walls": WALLS, "maze_agent_position": "0,0",
                                   "maze_target_position": "9,12"}),
    ("Maze-v0__on_target", "Maze-v0", {"maze_agent_position": "3,4", "maze_target_position": "3,4"}),
]


def registry() -> dict:
    recorded = {}

    def register(task_id, aliases, spec_cls, dm_cls, gymnasium_cls, max_episode_steps, **kwargs):
        if task_id in PREFIX:
            recorded[task_id] = dict(kwargs, aliases=list(aliases), spec_cls=spec_cls, dm_cls=dm_cls,
                                     gymnasium_cls=gymnasium_cls, max_episode_steps=max_episode_steps)

    stub = types.ModuleType("envpool.registration")
    stub.register = register
    pkg = types.ModuleType("envpool")
    pkg.registration = stub
    saved = {k: sys.modules.get(k) for k in ("envpool", "envpool.registration")}
    sys.modules["envpool"], sys.modules["envpool.registration"] = pkg, stub
    try:
        rel = "envpool/jumanji/registration.py"
        exec(compile(open(os.path.join(REF, rel)).read(), rel, "exec"), {"__name__": "golden"})
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return recorded


def build(tmp: str) -> str:
    exe = os.path.join(tmp, "driver")
    subprocess.run(["g++", "-std=c++17", "-O2", "-DNDEBUG", "-w", "-I", os.path.join(ROOT, "oracle", "ref_shims"),
                    "-I", REF, os.path.join(HERE, "jumanji_golden_driver.cc"), "-o", exe, "-lpthread"], check=True)
    return exe


def actions(i: int, puzzle: str, steps: int) -> np.ndarray:
    """Seeded actions, a few of them outside the bounds (the env clamps them)."""
    rng = np.random.default_rng(2000 + i)
    if puzzle == "Minesweeper":
        return rng.integers(-1, 11, size=(steps, N, 2)).astype(np.int32)
    if puzzle.startswith("RubiksCube"):
        a = np.stack([rng.integers(-1, 7, (steps, N)), rng.integers(0, 2, (steps, N)),
                      rng.integers(-1, 4, (steps, N))], axis=-1)
        return a.astype(np.int32)
    return rng.integers(-1, 5, size=(steps, N)).astype(np.int32)


def rollout(exe: str, tmp: str, i: int, name: str, tid: str, kw: dict, max_steps: int) -> dict:
    d = os.path.join(tmp, f"run{i}")
    os.makedirs(d)
    puzzle = PREFIX[tid]
    steps = max(MIN_STEPS, max_steps + 20)
    acts = actions(i, puzzle, steps)
    acts.tofile(os.path.join(d, "actions.bin"))
    seed = 300 + 17 * i
    args = [f"{k}={v}" for k, v in kw.items()]
    subprocess.run([exe, "run", puzzle, d, str(steps), os.path.join(d, "actions.bin"), "1", f"num_envs={N}",
                    f"seed={seed}"] + args, check=True)
    spec = json.loads(subprocess.run([exe, "spec", puzzle], check=True, capture_output=True, text=True).stdout)
    keys = open(os.path.join(d, "keys.txt")).read().split()
    dt = {k: np.dtype(s["dtype"]) for k, s in spec["state_spec"]}
    shp = {k: [x for x in s["shape"] if x != -1] for k, s in spec["state_spec"]}
    out = {}
    for k in keys:
        out[k] = np.fromfile(os.path.join(d, k + ".bin"), dtype=dt[k]).reshape(steps + 1, N, *shp[k])
    order = np.argsort(out["info:env_id"], axis=1, kind="stable")
    for k in keys:
        out[k] = np.take_along_axis(out[k], order.reshape(steps + 1, N, *([1] * len(shp[k]))), axis=1)
    assert (out["info:env_id"] == np.arange(N)).all()
    hidden = np.fromfile(os.path.join(d, "hidden.bin"), dtype=np.int32).reshape(steps + 1, N, -1)
    used = np.fromfile(os.path.join(d, "actions_used.bin"), dtype=np.int32).reshape(acts.shape)
    res = {k.replace(":", "__"): v for k, v in out.items()}
    res.update(actions=used, seed=np.int32(seed), hidden=hidden, config=np.array(json.dumps(kw)),
               task_id=np.array(tid))
    return {"name": name, "tid": tid, "spec": spec, "data": res}


def coverage(r: dict) -> set:
    g, puzzle = r["data"], PREFIX[r["tid"]]
    rew, done, trunc, el = g["reward"][1:], g["done"][1:], g["trunc"][1:], g["elapsed_step"][1:]
    prev_done = g["done"][:-1]
    stepped = ~prev_done  # rows that were a step (not an auto-reset)
    hid, act = g["hidden"], g["actions"]
    ev = set()
    if (g["elapsed_step"][1:] == 0).any():
        ev.add("auto_reset")
    if (g["done"][g["elapsed_step"] == 0]).any():
        ev.add("terminal_reset")
    end = done & stepped
    if puzzle == "Game2048" and end.any():
        ev.add("game_over")
    if puzzle == "Minesweeper":
        cell = np.clip(act[..., 0], 0, 9) * 10 + np.clip(act[..., 1], 0, 9)
        before = np.take_along_axis(hid[:-1, :, :100], cell[..., None], axis=2)[..., 0]
        mine = np.take_along_axis(hid[:-1, :, 100:200], cell[..., None], axis=2)[..., 0]
        if (end & (before == -1) & (mine == 1)).any():
            ev.add("mine")
        if (end & (before != -1)).any():
            ev.add("invalid")
        if (end & (rew == 1)).any():
            ev.add("win")
    if puzzle in ("SlidingTilePuzzle", "RubiksCube", "RubiksCubePartlyScrambled", "Maze"):
        limit = {"SlidingTilePuzzle": 500, "RubiksCube": 200, "RubiksCubePartlyScrambled": 20, "Maze": 100}[puzzle]
        if (end & (el == limit) & ~trunc & (g["step_type"][1:] == 2)).any():
            ev.add("time_limit")
        if puzzle == "SlidingTilePuzzle" and (end & (el < limit) & (g["info__prop_correctly_placed"][1:] == 1)).any():
            ev.add("solved")
        if puzzle != "SlidingTilePuzzle" and (end & (rew == 1)).any():
            ev.add("solved")
    if puzzle == "Snake":
        if (stepped & (rew == 1)).any():
            ev.add("fruit")
        moves = np.array([[-1, 0], [0, 1], [1, 0], [0, -1]])
        mv = moves[np.clip(act, 0, 3)]
        head = hid[:-1, :, 144:146]
        nxt = head + mv
        inside = (nxt >= 0).all(-1) & (nxt < 12).all(-1)
        if (end & ~inside).any():
            ev.add("wall")
        if (end & inside & (rew == 0)).any():
            ev.add("self")
    return ev


def main() -> None:
    reg = registry()
    assert sorted(reg) == sorted(PREFIX), sorted(reg)
    tmp = tempfile.mkdtemp(prefix="jumanji_golden_")
    try:
        exe = build(tmp)
        first = [(i, f) for i, f in enumerate(FIXTURES) if f[2].get("rubiks_cube_initial_cube", "") is not None]
        with ThreadPoolExecutor(8) as ex:
            runs = list(ex.map(lambda a: rollout(exe, tmp, a[0], *a[1], reg[a[1][1]]["max_episode_steps"]), first))
        # the partly-scrambled cube's configured start: env 1's first cube of the one-scramble fixture
        cube = next(r for r in runs if r["name"] == "RubiksCube-v0__scramble1")["data"]["obs__cube"][0, 1]
        assert cube.tolist() != np.repeat(np.arange(6), 9).reshape(6, 3, 3).tolist()
        for i, (name, tid, kw) in enumerate(FIXTURES):
            if kw.get("rubiks_cube_initial_cube", "") is None:
                kw = dict(kw, rubiks_cube_initial_cube=",".join(str(int(v)) for v in cube.ravel()))
                runs.append(rollout(exe, tmp, i, name, tid, kw, reg[tid]["max_episode_steps"]))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    seen = {}
    for r in runs:
        ev = coverage(r)
        assert "auto_reset" in ev, r["name"]
        seen.setdefault(PREFIX[r["tid"]], set()).update(ev)
    want = {"Game2048": {"game_over"}, "Minesweeper": {"mine", "win", "invalid"},
            "SlidingTilePuzzle": {"solved", "time_limit"}, "RubiksCube": {"solved", "time_limit"},
            "RubiksCubePartlyScrambled": {"solved", "time_limit"}, "Snake": {"fruit", "self", "wall"},
            "Maze": {"solved", "time_limit", "terminal_reset"}}
    for p, w in want.items():
        assert w <= seen[p], (p, w - seen[p])
    json.dump(reg, open(os.path.join(HERE, "jumanji_registry.json"), "w"), indent=1, sort_keys=True)
    json.dump({r["tid"]: r["spec"] for r in runs if r["name"] == r["tid"]},
              open(os.path.join(HERE, "jumanji_spec.json"), "w"), indent=1)
    total = 0
    for r in runs:
        path = os.path.join(HERE, f"jumanji_{r['name']}.npz")
        np.savez_compressed(path, **r["data"])
        total += os.path.getsize(path)
    print(len(runs), "fixtures,", total, "bytes; coverage:", {k: sorted(v) for k, v in seen.items()})


if __name__ == "__main__":
    main()
