"""Generates the MiniGrid fixtures from the reference itself.  Run on a machine that has the
reference tree (it is not on the GPU boxes):

    python tests/golden/make_minigrid_golden.py [/path/to/reference]

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


def steps_of(kw: dict) -> int:
    return max(MIN_STEPS, kw["max_episode_steps"] + 20)


def actions(i: int, action_max: int, steps: int) -> np.ndarray:
    rng = np.random.default_rng(1000 + i)
    a = rng.integers(0, action_max + 1, size=(steps, N)).astype(np.int32)
    fwd = rng.random((steps, N)) < 0.5
    a[fwd] = 2
    a[:, N - 1] = rng.integers(0, 2, steps)  # turns only: never ends before max_episode_steps
    return a


def rollout(exe: str, tmp: str, i: int, tid: str, kw: dict) -> dict:
    d = os.path.join(tmp, f"run{i}")
    os.makedirs(d)
    STEPS = steps_of(kw)
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
        steps = g["actions"].shape[0]
        rew, done, trunc, el = g["reward"][1:], g["done"][1:], g["trunc"][1:], g["elapsed_step"][1:]
        assert trunc.any(), (r["tid"], "no truncation at max_episode_steps")
        assert (el == 0).any(), (r["tid"], "no auto-reset")
        ev = seen.setdefault(env, set())
        if (rew > 0).any():
            ev.add("goal")
        if (rew < 0).any():
            ev.add("collision")
        # lava termination: an episode that ends, not truncated, without reward, with the agent on a lava cell
        h = int(g["height"])
        gr = g["grid"][1:].reshape(steps, N, -1, 3)
        pos = g["info__agent_pos"][1:]
        under = np.take_along_axis(gr[..., 0], (pos[..., 0] * h + pos[..., 1])[..., None], axis=2)[..., 0]
        if (done & ~trunc & (rew == 0) & (under == 9)).any():
            ev.add("lava")
        # an unlocked door: a door cell (type 4) in state open (0); DoorKey's door starts locked
        if ((gr[..., 0] == 4) & (gr[..., 2] == 0)).any():
            ev.add("unlock")
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
    main()
