"""Generates the render fixtures from the reference itself.  Run on a machine that has the reference tree (it is
not on the GPU boxes):

    python tests/golden/make_render_golden.py [/path/to/reference]

It compiles render_golden_driver.cc, which includes the reference's Jumanji puzzles and PGX board games in place
inside their own AsyncEnvPool, with the absl stand-ins of oracle/ref_shims (read only), into a temporary directory
outside the repository.  Then it writes data only, one file per game:

  tests/golden/render_<Game>.npz
      hidden     int32 [P, words]   the hidden state of P picked (run, step, env) states, in the word order of
                                    get_state after (elapsed step, done): the HIDDEN tables of
                                    make_jumanji_golden.py / make_pgx_golden.py, Hex as the sign of its labels
      sizes      int32 [S, 2]       the (width, height) asked for, SIZES below; resolved: what RenderSize made of them
      frame_<s>  uint8 [P, H, W, 3] what the reference's pool.Render returned for each state at size s
      picks      int32 [P, 3]       (run, step, env) of each state;  tags: JSON, what each state covers

Each game's pool is rolled with the driver's seeded policy; the states are picked from the roll-out so that together
they cover the game's tags (WANTED), which is asserted before anything is written.  The sizes are the smallest that
reach each arithmetic path: the defaults; 61 x 45 (odd, not square: uneven cell edges, rows of 183 bytes); 16 x 16
(radius floors, refused digits, rectangles inverted by their padding); 7 x 30 (higher than wide; RubiksCube's
face_side 1 with a negative origin); 1 x 1.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
SIZES = [(0, 0), (61, 45), (16, 16), (7, 30), (1, 1)]
LIMIT = os.path.getsize(os.path.join(HERE, "pgx_Hex-v1.npz"))  # no fixture larger than the largest one there is

# game -> runs of (config keys, envs, steps); a state of run r may only cover the tags WANTED lists for that run
RUNS = {
    "Game2048": [({"game2048_initial_board": ",".join(str(i) for i in range(16))}, 1, 0), ({}, 2, 60)],
    "Minesweeper": [({}, 2, 30)],
    "SlidingTilePuzzle": [({}, 2, 4)],
    "RubiksCube": [({}, 4, 8)],
    "Snake": [({}, 2, 120)],
    "Maze": [({}, 2, 60)],
    "TicTacToe": [({}, 2, 8)],
    "ConnectFour": [({}, 2, 20)],
    "Hex": [({}, 4, 80)],
    "Othello": [({}, 2, 30)],
}
WANTED = {
    "Game2048": [{"exponents_0_to_15"}, {"rolled_out"}],
    "Minesweeper": [{"unexplored", "zero", "count1", "count2", "count3"}],
    "SlidingTilePuzzle": [{"scrambled"}],
    "RubiksCube": [{"six_colours_in_one_row"}],
    "Snake": [{"length4", "head_on_border", "head_next_to_fruit"}],
    "Maze": [{"walls", "agent_on_border", "agent_next_to_target"}],
    "TicTacToe": [{"both_colours", "adjacent"}],
    "ConnectFour": [{"both_colours", "adjacent"}],
    "Hex": [{"both_colours", "adjacent", "last_cell"}],
    "Othello": [{"both_colours", "adjacent"}],
}
BOARD = {"TicTacToe": (3, 3, -1), "ConnectFour": (6, 7, -1), "Hex": (11, 11, 0), "Othello": (8, 8, 0)}


def tags(game: str, w: np.ndarray, last: bool) -> set:
    """What one state (its hidden words) shows."""
    t = set()
    if game == "Game2048":
        if sorted(w[:16]) == list(range(16)):
            t.add("exponents_0_to_15")
        if last and (w[:16] > 2).any():
            t.add("rolled_out")
    elif game == "Minesweeper":
        b = w[:100]
        t |= {name for name, v in (("unexplored", -1), ("zero", 0), ("count1", 1), ("count2", 2), ("count3", 3))
              if (b == v).any()}
    elif game == "SlidingTilePuzzle":
        if sorted(w[:25]) == list(range(25)) and list(w[:25]) != list(range(1, 25)) + [0]:
            t.add("scrambled")
    elif game == "RubiksCube":
        # the unfolded cube's middle strip: faces 1..4 side by side, one sticker row of it is 12 stickers
        cube = w[:54].reshape(6, 3, 3)
        if any(len(set(cube[1:5, r, :].ravel())) == 6 for r in range(3)):
            t.add("six_colours_in_one_row")
    elif game == "Snake":
        hr, hc, fr, fc, length = w[144], w[145], w[148], w[149], w[150]
        if length >= 4:
            t.add("length4")
        if hr in (0, 11) or hc in (0, 11):
            t.add("head_on_border")
        if abs(hr - fr) + abs(hc - fc) == 1:
            t.add("head_next_to_fruit")
    elif game == "Maze":
        ar, ac, tr, tc = w[100:104]
        if w[:100].any():
            t.add("walls")
        if ar in (0, 9) or ac in (0, 9):
            t.add("agent_on_border")
        if abs(ar - tr) + abs(ac - tc) == 1:
            t.add("agent_next_to_target")
    else:
        rows, cols, empty = BOARD[game]
        b = w[:rows * cols].reshape(rows, cols)
        stone = b != empty
        if len(set(b[stone])) == 2:
            t.add("both_colours")
        if (stone[:, :-1] & stone[:, 1:]).any():
            t.add("adjacent")
        if game == "Hex" and stone[10, 10]:
            t.add("last_cell")
    return t


def build(tmp: str) -> str:
    exe = os.path.join(tmp, "driver")
    subprocess.run(["g++", "-std=c++17", "-O2", "-DNDEBUG", "-w", "-I", os.path.join(ROOT, "oracle", "ref_shims"),
                    "-I", REF, os.path.join(HERE, "render_golden_driver.cc"), "-o", exe, "-lpthread"], check=True)
    return exe


def roll(exe: str, tmp: str, game: str, kw: dict, n: int, steps: int, seed: int, picks: list):
    d = tempfile.mkdtemp(dir=tmp)
    sizes = ",".join(f"{w}x{h}" for w, h in SIZES)
    pk = ",".join(f"{t}:{e}" for t, e in picks) or "-"
    subprocess.run([exe, "run", game, d, str(n), str(steps), str(seed), str(10007 * seed + 1), pk, sizes] +
                   [f"{k}={v}" for k, v in kw.items()], check=True)
    hidden = np.fromfile(os.path.join(d, "hidden.bin"), dtype=np.int32).reshape(steps + 1, n, -1)
    if not picks:
        return hidden, None, None
    resolved = np.loadtxt(os.path.join(d, "sizes.txt"), dtype=np.int32).reshape(len(SIZES), 2)
    frames = [[np.fromfile(os.path.join(d, f"frame_{p}_{s}.bin"), dtype=np.uint8).reshape(h, w, 3)
               for p in range(len(picks))] for s, (w, h) in enumerate(resolved)]
    return hidden, resolved, frames


def choose(game: str, run: int, hidden: np.ndarray) -> list:
    """A few states, earliest first, that cover the run's tags (greedy); None if the roll-out does not."""
    want = set(WANTED[game][run])
    steps1, n, _ = hidden.shape
    shown = {(t, e): tags(game, hidden[t, e], t == steps1 - 1) & want for t in range(steps1) for e in range(n)}
    picks = []
    while want:
        best = max(shown, key=lambda k: (len(shown[k] & want), -k[0], -k[1]))
        if not shown[best] & want:
            return None
        picks.append(best)
        want -= shown[best]
    # ... and for variety every env where the roll-out left it
    return sorted(set(picks) | {(steps1 - 1, e) for e in range(n)})


def main() -> None:
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        for game, runs in RUNS.items():
            hid, where, frames, resolved, shown = [], [], [[] for _ in SIZES], None, []
            for r, (kw, n, steps) in enumerate(runs):
                for seed in range(1, 200):
                    hidden, _, _ = roll(exe, tmp, game, kw, n, steps, seed, [])
                    picks = choose(game, r, hidden)
                    if picks is not None:
                        break
                else:
                    raise SystemExit(f"{game} run {r}: no seed covers {sorted(WANTED[game][r])}")
                again, resolved, fr = roll(exe, tmp, game, kw, n, steps, seed, picks)
                assert np.array_equal(again, hidden), game
                for p, (t, e) in enumerate(picks):
                    hid.append(hidden[t, e])
                    where.append((r, t, e))
                    shown.append(sorted(tags(game, hidden[t, e], t == steps)))
                    for s in range(len(SIZES)):
                        frames[s].append(fr[s][p])
                print(f"{game} run {r}: seed {seed}, states {picks}")
            covered = set().union(*shown)
            assert covered >= set().union(*WANTED[game]), (game, covered)
            g = {"hidden": np.stack(hid).astype(np.int32), "picks": np.array(where, np.int32),
                 "sizes": np.array(SIZES, np.int32), "resolved": resolved, "tags": np.array(json.dumps(shown))}
            for s in range(len(SIZES)):
                g[f"frame_{s}"] = np.stack(frames[s])
            out[game] = g
    for game, g in out.items():
        path = os.path.join(HERE, f"render_{game}.npz")
        np.savez_compressed(path, **g)
        assert os.path.getsize(path) <= LIMIT, (path, os.path.getsize(path))
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
