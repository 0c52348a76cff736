"""Generates the PGX board-game fixtures from the reference itself.  Run on a machine that has the reference tree
(it is not on the GPU boxes):

    python tests/golden/make_pgx_golden.py [--scripted] [/path/to/reference]

It compiles pgx_golden_driver.cc, which includes the reference's envpool/pgx/board_games.h in place inside its own
AsyncEnvPool (max_num_players = 2), with the absl stand-ins of oracle/ref_shims (read only), into a temporary
directory outside the repository.  Then it writes data only:

  tests/golden/pgx_registry.json   the `register` kwargs of TicTacToe-v1, ConnectFour-v1, Hex-v1, Othello-v1
  tests/golden/pgx_spec.json       per id: DefaultConfig key set / defaults, state and action specs
  tests/golden/pgx_<name>.npz      n envs x `steps` actions picked online by the driver's seeded policy from each
                                   env's legal action mask (a per-env share of them illegal): every state key after
                                   the reset and after every step as [steps + 1, n, <per-env row>] (a per-player
                                   key's row is its [2, ...] block), the hidden state of every env after each of
                                   them (`hidden`, int32 words, HIDDEN below), the actions (`actions` [steps, n]),
                                   the seed and max_episode_steps

  tests/golden/pgx_<id>__scripted.npz
                                   the same arrays for scripted actions (the driver's `replay` mode): legal games
                                   from reset found by pgx_scripted.py with the scalar restatement of the rules,
                                   whose required content (every ConnectFour line, Othello wipe-outs, long Hex
                                   chains, ...: see there) is asserted on the reference's output before writing.
                                   --scripted writes these four files only and leaves every other file as it is.

<name> is the id, or <id>__trunc for a run with a small max_episode_steps.  The seeds are searched until a run
covers, per game: a win by each seat; a draw (TicTacToe, ConnectFour, Othello); an illegal-move ending of each
kind; a legal Hex swap; a legal Othello pass and an Othello end by a double pass or a wipe-out; an auto-reset; and
for the __trunc runs a truncated ending.  Coverage is asserted before anything is written.
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import types

import numpy as np

import pgx_scripted

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
ARGS = [a for a in sys.argv[1:] if a != "--scripted"]
ONLY_SCRIPTED = "--scripted" in sys.argv[1:]
REF = ARGS[0] if ARGS else "/root/reference"
SCRIPTED_SEED, SCRIPTED_ENVS = 7, 4
GAME = {"TicTacToe-v1": "TicTacToe", "ConnectFour-v1": "ConnectFour", "Hex-v1": "Hex", "Othello-v1": "Othello"}
ACTIONS = {"TicTacToe": 9, "ConnectFour": 7, "Hex": 122, "Othello": 65}
# int32 words of the driver's hidden state per env
HIDDEN = {"TicTacToe": "board[9] color current_player", "ConnectFour": "board[42] color current_player",
          "Hex": "board[121] (union-find labels) step_count player_order[0]",
          "Othello": "board[64] turn current_player passed"}
# (fixture name, id, envs, steps, illegal permille of the second half of the envs, max_episode_steps)
FIXTURES = [
    ("TicTacToe-v1", "TicTacToe-v1", 8, 160, 150, None),
    ("TicTacToe-v1__trunc", "TicTacToe-v1", 4, 40, 0, 6),
    ("ConnectFour-v1", "ConnectFour-v1", 8, 700, 40, None),
    ("ConnectFour-v1__trunc", "ConnectFour-v1", 4, 80, 0, 12),
    ("Hex-v1", "Hex-v1", 8, 500, 12, None),
    ("Hex-v1__trunc", "Hex-v1", 4, 120, 0, 30),
    ("Othello-v1", "Othello-v1", 8, 900, 12, None),
    ("Othello-v1__trunc", "Othello-v1", 4, 150, 0, 40),
]
INT_MAX = 2**31 - 1


def registry() -> dict:
    recorded = {}

    def register(task_id, **kwargs):
        if task_id in GAME:
            recorded[task_id] = kwargs

    stub = types.ModuleType("envpool.registration")
    stub.register = register
    pkg = types.ModuleType("envpool")
    pkg.registration = stub
    saved = {k: sys.modules.get(k) for k in ("envpool", "envpool.registration")}
    sys.modules["envpool"], sys.modules["envpool.registration"] = pkg, stub
    try:
        rel = "envpool/pgx/registration.py"
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
                    "-I", REF, os.path.join(HERE, "pgx_golden_driver.cc"), "-o", exe, "-lpthread"], check=True)
    return exe


def rollout(exe: str, tmp: str, spec: dict, game: str, n: int, steps: int, permille: int, limit, seed: int,
            script=None) -> dict:
    d = tempfile.mkdtemp(dir=tmp)
    per_env = [0 if e < n // 2 else permille for e in range(n)]
    args = [exe, "run", game, d, str(n), str(steps), str(seed), str(10007 * seed + 1)] + [str(p) for p in per_env]
    if script is not None:
        np.ascontiguousarray(script, np.int32).tofile(os.path.join(d, "script.bin"))
        args = [exe, "replay", game, d, str(n), str(steps), str(seed), os.path.join(d, "script.bin")]
    if limit is not None:
        args.append(f"max_episode_steps={limit}")
    subprocess.run(args, check=True)
    out = {}
    dtypes = {k: s["dtype"] for k, s in spec["state_spec"]}
    for line in open(os.path.join(d, "keys.txt")):
        key, per = line.split()
        shape = [abs(x) for x in dict(spec["state_spec"])[key]["shape"]]
        if int(per) == 2:
            shape[0] = 2
        raw = np.fromfile(os.path.join(d, key + ".bin"), dtype=dtypes[key])
        out[key] = raw.reshape(steps + 1, n, *shape)
    out["actions"] = np.fromfile(os.path.join(d, "actions.bin"), dtype=np.int32).reshape(steps, n)
    out["hidden"] = np.fromfile(os.path.join(d, "hidden.bin"), dtype=np.int32).reshape(steps + 1, n, -1)
    out["seed"] = np.int32(seed)
    out["max_episode_steps"] = np.int32(INT_MAX if limit is None else limit)
    shutil.rmtree(d)
    return out


def coverage(game: str, g: dict) -> set:
    """What a run shows (the tags `wanted` asks for)."""
    A = ACTIONS[game]
    tags = set()
    done, mask, rew, acts = g["done"], g["info:legal_action_mask"], g["reward"], g["actions"]
    steps, n = acts.shape
    for t in range(steps):
        for e in range(n):
            if done[t, e]:
                continue
            a = int(acts[t, e])
            legal = 0 <= a < A and bool(mask[t, e, a])
            r = tuple(float(x) for x in rew[t + 1, e])
            if not legal:
                kind = "neg" if a < 0 else "past" if a >= A else "swap" if (game == "Hex" and a == 121) else \
                    "pass" if (game == "Othello" and a == 64) else "occupied"
                assert done[t + 1, e]
                tags.add("illegal_" + kind)
                continue
            if game == "Hex" and a == 121:
                tags.add("swap")
            if game == "Othello" and a == 64:
                tags.add("pass")
            if done[t + 1, e]:
                tags.add({(1.0, -1.0): "win0", (-1.0, 1.0): "win1", (0.0, 0.0): "draw"}[r])
                if game == "Othello":
                    board = g["info:board"][t + 1, e]
                    if a == 64:
                        tags.add("double_pass")
                    if (board == 0).any() and not (board == 1).any():
                        tags.add("wipe_out")
            if t + 1 <= steps and g["elapsed_step"][t + 1, e] == 0:
                tags.add("auto_reset")
        if g["trunc"][t + 1].any():
            tags.add("trunc")
    for t in range(1, steps + 1):
        if (g["elapsed_step"][t] == 0).any():
            tags.add("auto_reset")
    return tags


def wanted(game: str, trunc: bool) -> set:
    if trunc:
        return {"trunc", "auto_reset"}
    w = {"win0", "win1", "auto_reset", "illegal_neg", "illegal_past", "illegal_occupied"}
    if game != "Hex":
        w.add("draw")
    if game == "Hex":
        w |= {"swap", "illegal_swap"}
    if game == "Othello":
        w |= {"pass", "illegal_pass", "end_by_pass_or_wipe_out"}
    return w


def main() -> None:
    reg = registry()
    assert sorted(reg) == sorted(GAME), reg
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        specs = {}
        for tid, game in GAME.items():
            specs[tid] = json.loads(subprocess.run([exe, "spec", game], check=True, capture_output=True,
                                                   text=True).stdout)
        runs = {}
        for name, tid, n, steps, permille, limit in ([] if ONLY_SCRIPTED else FIXTURES):
            game = GAME[tid]
            want = wanted(game, limit is not None)
            for seed in range(1, 400):
                g = rollout(exe, tmp, specs[tid], game, n, steps, permille, limit, seed)
                got = coverage(game, g)
                if got & {"double_pass", "wipe_out"}:
                    got.add("end_by_pass_or_wipe_out")
                if want <= got:
                    break
            else:
                raise SystemExit(f"{name}: no seed covers {sorted(want)}")
            print(f"{name}: seed {seed}, covers {sorted(got)}")
            runs[name] = g
        for tid, game in GAME.items():
            acts = pgx_scripted.script(game, SCRIPTED_SEED, SCRIPTED_ENVS)
            g = rollout(exe, tmp, specs[tid], game, SCRIPTED_ENVS, len(acts), 0, None, SCRIPTED_SEED, script=acts)
            assert np.array_equal(g["actions"], acts)
            got = pgx_scripted.check(game, g)
            print(f"{tid}__scripted: {len(acts)} steps x {SCRIPTED_ENVS} envs, covers",
                  {k: (len(v) if isinstance(v, set) else v) for k, v in got.items() if v})
            runs[f"{tid}__scripted"] = g
    if not ONLY_SCRIPTED:
        json.dump(reg, open(os.path.join(HERE, "pgx_registry.json"), "w"), indent=1, sort_keys=True)
        json.dump(specs, open(os.path.join(HERE, "pgx_spec.json"), "w"), indent=1)
    for name, g in runs.items():
        np.savez_compressed(os.path.join(HERE, f"pgx_{name}.npz"), **g)
    # a scripted fixture is no larger than the largest of the others
    largest = max(os.path.getsize(os.path.join(HERE, f"pgx_{name}.npz")) for name, *_ in FIXTURES)
    for tid in GAME:
        assert os.path.getsize(os.path.join(HERE, f"pgx_{tid}__scripted.npz")) <= largest, tid

if __name__ == "__main__":
    main()
