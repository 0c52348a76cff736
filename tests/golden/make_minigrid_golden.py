"""Generates the MiniGrid fixtures from the reference itself.  Run on a machine that has the
reference tree (it is not on the GPU boxes):

    python tests/golden/make_minigrid_golden.py [/path/to/reference]            the 30 registered ids
    python tests/golden/make_minigrid_golden.py [/path/to/reference] --options  the option cases only

It compiles the reference's MiniGrid translation units (the `minigrid_env` list of
envpool/minigrid/BUILD) in place, plus minigrid_golden_driver.cc, with the absl stand-ins of
oracle/ref_shims (read only) and the OpenCV stub under minigrid_stub/ (rendering is not
recorded), into a temporary directory outside the repository.  Then it writes data only:

  tests/golden/minigrid_registry.json  the `register` kwargs of the 30 navigation ids
  tests/golden/minigrid_spec.json      per id: DefaultConfig key set / defaults, state and action specs
  tests/golden/minigrid_<id>.npz       8 envs x max(300, max_episode_steps + 20) seeded actions: envs 0-6
                                       biased towards `forward` (so that episodes end), env 7 only turning
                                       (so that it runs into max_episode_steps and auto-resets); every state
                                       key after the reset and after every step (rows in env id order), and
                                       after each of them the DebugState of every env (grid encoding x-major
                                       like DebugState::grid, agent, carried object, obstacle positions)

Before writing anything it asserts coverage: every id has a truncation at max_episode_steps and an
auto-reset; every env_name has a goal reward; lava termination (the agent ends on a lava cell) wherever
there is lava (DistShift, LavaGap, LavaCrossing); the -1 collision for Dynamic-Obstacles; a door unlocked
for DoorKey.

With --options it leaves all of the above alone and writes the configs outside the registered ids
(OPTION_CASES below: other grid sides, non-square DistShift, fixed / random starts, every river count,
wall-type LavaGap, obstacle counts 0..8, short max_episode_steps):

  tests/golden/minigrid_opt__<case>.npz    the same arrays, 8 envs x max(150, max_episode_steps + 20) steps,
                                           seeds and action streams of case index 100 + position in the table
  tests/golden/minigrid_option_cases.json  per case: the kwargs and the reference's spec for that config

Each case asserts the events listed with it (and a truncation and an auto-reset) before anything is written.
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
ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
REF = ARGS[0] if ARGS else "/root/reference"
N, MIN_STEPS, OPT_MIN_STEPS, OPT_INDEX0 = 8, 300, 150, 100
TUS = ["babyai_core", "babyai_env", "babyai_goto_tasks", "babyai_instr", "babyai_open_tasks",
       "babyai_pickup_tasks", "babyai_tasks", "babyai_unlock_tasks", "minigrid_core", "minigrid_env",
       "minigrid_render", "minigrid_room_tasks", "minigrid_task_factory", "minigrid_tasks",
       "minigrid_wfc_tasks"]
ENV_NAMES = {"empty", "doorkey", "distshift", "crossing", "lava_gap", "dynamic_obstacles", "four_rooms"}
DBG_HEAD = 26  # int32 words per env in front of the grid (minigrid_golden_driver.cc)


def registry() -> dict:
    recorded = {}

    def register(task_id, import_path, spec_cls, dm_cls, gymnasium_cls, **kwargs):
        if kwargs.get("env_name") in ENV_NAMES:
            recorded[task_id] = {k: list(v) if isinstance(v, tuple) else v for k, v in kwargs.items()}

    stub = types.ModuleType("envpool.registration")
    stub.register = register
    pkg = types.ModuleType("envpool")
    pkg.registration = stub
    saved = {k: sys.modules.get(k) for k in ("envpool", "envpool.registration")}
    sys.modules["envpool"], sys.modules["envpool.registration"] = pkg, stub
    try:
        rel = "envpool/minigrid/registration.py"
        exec(compile(open(os.path.join(REF, rel)).read(), rel, "exec"), {"__name__": "golden"})
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return recorded


def driver_args(kw: dict) -> list:
    out = []
    for k, v in kw.items():
        out.append(f"{k}={v[0]},{v[1]}" if isinstance(v, list) else f"{k}={v}")
    return out


def build(tmp: str) -> str:
    inc = ["-I", os.path.join(ROOT, "oracle", "ref_shims"), "-I", os.path.join(HERE, "minigrid_stub"), "-I", REF]
    flags = ["g++", "-std=c++17", "-O2", "-DNDEBUG", "-w"] + inc

    def cc(tu):
        obj = os.path.join(tmp, tu + ".o")
        subprocess.run(flags + ["-c", os.path.join(REF, "envpool", "minigrid", "impl", tu + ".cc"), "-o", obj],
                       check=True)
        return obj

    with ThreadPoolExecutor(8) as ex:
        objs = list(ex.map(cc, TUS))
    exe = os.path.join(tmp, "driver")
    subprocess.run(flags + [os.path.join(HERE, "minigrid_golden_driver.cc")] + objs + ["-o", exe, "-lpthread"],
                   check=True)
    return exe


def steps_of(kw: dict, min_steps: int = MIN_STEPS) -> int:
    return max(min_steps, kw["max_episode_steps"] + 20)


def actions(i: int, action_max: int, steps: int) -> np.ndarray:
    rng = np.random.default_rng(1000 + i)
    a = rng.integers(0, action_max + 1, size=(steps, N)).astype(np.int32)
    fwd = rng.random((steps, N)) < 0.5
    a[fwd] = 2
    a[:, N - 1] = rng.integers(0, 2, steps)  # turns only: never ends before max_episode_steps
    return a


def rollout(exe: str, tmp: str, i: int, tid: str, kw: dict, min_steps: int = MIN_STEPS) -> dict:
    d = os.path.join(tmp, f"run{i}")
    os.makedirs(d)
    STEPS = steps_of(kw, min_steps)
    acts = actions(i, kw.get("action_max", 6), STEPS)
    acts.tofile(os.path.join(d, "actions.bin"))
    seed = 100 + 17 * i
    subprocess.run([exe, "run", d, str(STEPS), os.path.join(d, "actions.bin"), f"num_envs={N}", f"seed={seed}"]
                   + driver_args(kw), check=True)
    spec = json.loads(subprocess.run([exe, "spec"] + driver_args(kw), check=True, capture_output=True,
                                     text=True).stdout)
    keys = open(os.path.join(d, "keys.txt")).read().split()
    dt = {k: np.dtype(s["dtype"]) for k, s in spec["state_spec"]}
    shp = {k: [x for x in s["shape"] if x != -1] for k, s in spec["state_spec"]}
    out = {}
    for k in keys:
        a = np.fromfile(os.path.join(d, k + ".bin"), dtype=dt[k]).reshape(STEPS + 1, N, *shp[k])
        out[k] = a
    order = np.argsort(out["info:env_id"], axis=1, kind="stable")
    for k in keys:
        out[k] = np.take_along_axis(out[k], order.reshape(STEPS + 1, N, *([1] * len(shp[k]))), axis=1)
    assert (out["info:env_id"] == np.arange(N)).all()
    raw = np.fromfile(os.path.join(d, "debug.bin"), dtype=np.uint8)
    w, h = np.frombuffer(raw[:8].tobytes(), dtype=np.int32)
    rec = DBG_HEAD * 4 + w * h * 3
    raw = raw.reshape(STEPS + 1, N, rec)
    head = np.frombuffer(raw[:, :, :DBG_HEAD * 4].tobytes(), dtype=np.int32).reshape(STEPS + 1, N, DBG_HEAD)
    res = {k.replace(":", "__"): v for k, v in out.items()}
    res.update(actions=acts, seed=np.int32(seed), width=np.int32(w), height=np.int32(h),
               grid=raw[:, :, DBG_HEAD * 4:].copy(), agent=head[:, :, 2:5].copy(),
               carrying=head[:, :, 5:8].copy(), obstacles=head[:, :, 9:25].copy())
    return {"tid": tid, "spec": spec, "data": res}


def events(g: dict) -> set:
    """What a rollout shows: goal (a positive reward), collision (a negative one), lava (an episode that ends,
    not truncated, without reward, with the agent on a lava cell), unlock (a door cell in state open)."""
    ev = set()
    steps = g["actions"].shape[0]
    rew, done, trunc = g["reward"][1:], g["done"][1:], g["trunc"][1:]
    if (rew > 0).any():
        ev.add("goal")
    if (rew < 0).any():
        ev.add("collision")
    h = int(g["height"])
    gr = g["grid"][1:].reshape(steps, N, -1, 3)
    pos = g["info__agent_pos"][1:]
    under = np.take_along_axis(gr[..., 0], (pos[..., 0] * h + pos[..., 1])[..., None], axis=2)[..., 0]
    if (done & ~trunc & (rew == 0) & (under == 9)).any():
        ev.add("lava")
    # an unlocked door: a door cell (type 4) in state open (0); DoorKey's door starts locked
    if ((gr[..., 0] == 4) & (gr[..., 2] == 0)).any():
        ev.add("unlock")
    return ev


# name -> (driver kwargs, events the rollout must show besides a truncation and an auto-reset,
#          number of auto-resets where the config leaves nothing but truncations, N * (steps // (mes + 1)), or None)
# The position in the table is the case's index: it sets the seed and the action stream.
OPTION_CASES = {
    "empty7_start": (dict(env_name="empty", size=7, agent_start_pos=[3, 2], agent_start_dir=3,
                          max_episode_steps=50), {"goal"}, None),
    "empty19_rand": (dict(env_name="empty", size=19, agent_start_pos=[-1, -1], max_episode_steps=100),
                     {"goal"}, None),
    "empty13_ongoal": (dict(env_name="empty", size=13, agent_start_pos=[11, 11], agent_start_dir=1,
                            max_episode_steps=60), {"goal"}, None),
    "empty5_mes1": (dict(env_name="empty", size=5, max_episode_steps=1), set(), None),
    "empty5_mes2": (dict(env_name="empty", size=5, max_episode_steps=2), set(), None),
    "empty6_mes7": (dict(env_name="empty", size=6, max_episode_steps=7), set(), None),
    "doorkey7": (dict(env_name="doorkey", size=7, max_episode_steps=25), set(), 40),
    "doorkey19": (dict(env_name="doorkey", size=19, max_episode_steps=40), set(), 24),
    "dist12x9": (dict(env_name="distshift", width=12, height=9, strip2_row=5, max_episode_steps=80),
                 {"lava"}, None),
    "dist7x5_rand": (dict(env_name="distshift", width=7, height=5, strip2_row=3, agent_start_pos=[-1, -1],
                          max_episode_steps=40), {"goal", "lava"}, None),
    # both lava strips in one row
    "dist19x5_s1": (dict(env_name="distshift", width=19, height=5, strip2_row=1, max_episode_steps=80),
                    {"lava"}, None),
    # no lava at all: the strips are width - 6 < 0 cells long
    "dist5x19": (dict(env_name="distshift", width=5, height=19, strip2_row=17, agent_start_pos=[3, 17],
                      agent_start_dir=2, max_episode_steps=30), set(), None),
    # the agent starts on a lava cell
    "dist_onlava": (dict(env_name="distshift", width=9, height=7, agent_start_pos=[3, 2], max_episode_steps=40),
                    {"lava"}, None),
    # num_crossings = every river of the size, up to the 16 of size 19
    "cross5n2": (dict(env_name="crossing", size=5, num_crossings=2, obstacle_type="lava", max_episode_steps=60),
                 {"goal", "lava"}, None),
    "cross7n4w": (dict(env_name="crossing", size=7, num_crossings=4, obstacle_type="wall", max_episode_steps=30),
                  {"goal"}, None),
    "cross9n6": (dict(env_name="crossing", size=9, num_crossings=6, obstacle_type="lava", max_episode_steps=40),
                 {"lava"}, None),
    "cross13n7w": (dict(env_name="crossing", size=13, num_crossings=7, obstacle_type="wall",
                        max_episode_steps=30), set(), 32),
    "cross15n12w": (dict(env_name="crossing", size=15, num_crossings=12, obstacle_type="wall",
                         max_episode_steps=30), set(), 32),
    "cross19n16": (dict(env_name="crossing", size=19, num_crossings=16, obstacle_type="lava",
                        max_episode_steps=200), {"lava"}, None),
    "cross19n1": (dict(env_name="crossing", size=19, num_crossings=1, obstacle_type="wall",
                       max_episode_steps=30), set(), 32),
    "gap5w": (dict(env_name="lava_gap", size=5, obstacle_type="wall", max_episode_steps=40), {"goal"}, None),
    "gap19w": (dict(env_name="lava_gap", size=19, obstacle_type="wall", max_episode_steps=30), set(), 32),
    "gap12": (dict(env_name="lava_gap", size=12, obstacle_type="lava", max_episode_steps=100),
              {"goal", "lava"}, None),
    "dyn7n0": (dict(env_name="dynamic_obstacles", size=7, n_obstacles=0, action_max=2, max_episode_steps=60),
               {"goal", "collision"}, None),
    # 8 obstacles: the limit of the packing
    "dyn16n8": (dict(env_name="dynamic_obstacles", size=16, n_obstacles=8, action_max=2, max_episode_steps=100),
                {"collision"}, None),
    # 8 asked for on a 5 x 5 grid: the reference clamps to size / 2 = 2
    "dyn5n8": (dict(env_name="dynamic_obstacles", size=5, n_obstacles=8, action_max=2, max_episode_steps=40),
               {"goal", "collision"}, None),
    "dyn10n6rand": (dict(env_name="dynamic_obstacles", size=10, n_obstacles=6, agent_start_pos=[-1, -1],
                         action_max=2, max_episode_steps=80), {"goal", "collision"}, None),
    # pickup / drop / toggle next to the balls
    "dyn6n4_act6": (dict(env_name="dynamic_obstacles", size=6, n_obstacles=4, action_max=6, max_episode_steps=80),
                    {"goal", "collision"}, None),
    "dyn9n5mid": (dict(env_name="dynamic_obstacles", size=9, n_obstacles=5, agent_start_pos=[4, 4],
                       agent_start_dir=2, action_max=2, max_episode_steps=80), {"goal", "collision"}, None),
}
# trunc on every step at which elapsed_step reaches max_episode_steps, checked on the env that only turns
SHORT_EPISODES = ("empty5_mes1", "empty5_mes2", "empty6_mes7")


def options_main() -> None:
    """The option cases only: nothing of the 30 ids is read or rewritten."""
    assert len(OPTION_CASES) == 29
    tmp = tempfile.mkdtemp(prefix="minigrid_golden_")
    try:
        exe = build(tmp)
        jobs = [(OPT_INDEX0 + k, name, kw, OPT_MIN_STEPS) for k, (name, (kw, _, _)) in enumerate(OPTION_CASES.items())]
        with ThreadPoolExecutor(8) as ex:
            runs = list(ex.map(lambda a: rollout(exe, tmp, *a), jobs))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    for r in runs:
        name, g = r["tid"], r["data"]
        kw, want, resets = OPTION_CASES[name]
        mes = kw["max_episode_steps"]
        assert g["actions"].shape[0] == max(OPT_MIN_STEPS, mes + 20), name
        trunc, el = g["trunc"][1:], g["elapsed_step"][1:]
        assert trunc.any(), (name, "no truncation at max_episode_steps")
        assert (el == 0).any(), (name, "no auto-reset")
        got = events(g)
        assert want <= got, (name, want - got)
        n_resets = int((el == 0).sum())
        assert resets is None or n_resets == resets == N * (g["actions"].shape[0] // (mes + 1)), (name, n_resets)
        if name in SHORT_EPISODES:
            assert np.array_equal(trunc[:, N - 1], el[:, N - 1] == mes), name
            assert trunc[:, N - 1].sum() == g["actions"].shape[0] // (mes + 1), name
        print(name, sorted(got), "resets", n_resets, "truncs", int(trunc.sum()))
    total = 0
    for r in runs:
        path = os.path.join(HERE, f"minigrid_opt__{r['tid']}.npz")
        np.savez_compressed(path, **r["data"])
        size = os.path.getsize(path)
        assert size < 100_000, (r["tid"], size)
        total += size
    assert total < 1_000_000, total
    table = {r["tid"]: {"kwargs": OPTION_CASES[r["tid"]][0], "spec": r["spec"]} for r in runs}
    with open(os.path.join(HERE, "minigrid_option_cases.json"), "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in table.items()) + "\n}\n")
    print(len(runs), "option cases,", total, "bytes of fixtures")


def main() -> None:
    reg = registry()
    assert len(reg) == 30, sorted(reg)
    tmp = tempfile.mkdtemp(prefix="minigrid_golden_")
    try:
        exe = build(tmp)
        with ThreadPoolExecutor(8) as ex:
            runs = list(ex.map(lambda a: rollout(exe, tmp, *a), [(i, t, reg[t]) for i, t in enumerate(sorted(reg))]))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    # coverage: per id, then per env_name over its ids
    seen = {}
    for r in runs:
        g, kw = r["data"], reg[r["tid"]]
        env = kw["env_name"]
        trunc, el = g["trunc"][1:], g["elapsed_step"][1:]
        assert trunc.any(), (r["tid"], "no truncation at max_episode_steps")
        assert (el == 0).any(), (r["tid"], "no auto-reset")
        seen.setdefault(env, set()).update(events(g))
    want = {"empty": {"goal"}, "doorkey": {"goal", "unlock"}, "distshift": {"goal", "lava"},
            "crossing": {"goal", "lava"}, "lava_gap": {"goal", "lava"},
            "dynamic_obstacles": {"goal", "collision"}, "four_rooms": {"goal"}}
    for env, w in want.items():
        assert w <= seen[env], (env, w - seen[env])
    json.dump(reg, open(os.path.join(HERE, "minigrid_registry.json"), "w"), indent=1, sort_keys=True)
    json.dump({r["tid"]: r["spec"] for r in runs}, open(os.path.join(HERE, "minigrid_spec.json"), "w"), indent=1)
    total = 0
    for r in runs:
        path = os.path.join(HERE, f"minigrid_{r['tid']}.npz")
        np.savez_compressed(path, **r["data"])
        total += os.path.getsize(path)
    print(len(runs), "ids,", total, "bytes of fixtures; coverage:", {k: sorted(v) for k, v in seen.items()})


if __name__ == "__main__":
    options_main() if "--options" in sys.argv[1:] else main()
