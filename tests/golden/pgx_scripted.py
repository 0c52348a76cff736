"""The scripted PGX fixtures (pgx_<id>__scripted.npz): legal games from reset, found by searching with the scalar
restatement of the rules (tests/pgx_rules_ref.py), that make_pgx_golden.py replays through the reference itself.
`script(game, seed, n)` returns actions[steps][n]; `coverage(game, g)` says what a recorded run shows, and
`check(game, g)` asserts the required content on the reference's own output before anything is written:

  TicTacToe    every one of the 8 lines as the winning line for each seat, 3 draws
  ConnectFour  every one of the 69 lines as a game-ending line, wins by both colors, 3 draws, a move on a full
               column in each of the 7 columns
  Othello      2 wipe-outs, 3 games ended by a second pass, 2 ties, a capture of run length 6 along a row, a column
               and a main diagonal, a move onto an own cell and onto an opponent's cell, each where a capture scan
               from the cell succeeds and where none does
  Hex          a legal swap from 30 first cells (the corners and the main diagonal among them), a win by each
               color with a group of at least 30 stones, a placement on an own and on an opponent's cell

An env plays its games one after the other; the action after a game's end is ignored by the auto-reset.  Which seat
moves first is the env generator's first bit per reset (mt19937 seeded with seed + env id), read here from numpy's
generator of the same seeding.  Searches run until the content is found; none samples a fixed count.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pgx_rules_ref as R  # noqa: E402

TTT_LINES = R.TTT_LINES


def c4_lines():
    lines = []
    for dr, dc in ((0, 1), (1, 0), (1, 1), (1, -1)):
        for r in range(6):
            for c in range(7):
                cells = [(r + dr * k, c + dc * k) for k in range(4)]
                if all(0 <= rr < 6 and 0 <= cc < 7 for rr, cc in cells):
                    lines.append(tuple(sorted(rr * 7 + cc for rr, cc in cells)))
    assert len(set(lines)) == 69
    return lines


def coins(seed, env, count):
    return [int(x) & 1 for x in np.random.RandomState(seed + env)._bit_generator.random_raw(count)]


# --------------------------------------------------------------------------------------------------------------- searches
def ttt_game(line, color):
    """A legal game that `color` wins on `line` (None: a draw), by depth-first search."""
    def go(p, acts):
        if p.done:
            won = [c for c in (0, 1) if R.ttt_won(p.board, c)]
            if line is None:
                return acts if not won else None
            ok = won == [color] and all(p.board[i] == color for i in line) and acts[-1] in line
            return acts if ok else None
        for a in range(9):
            if not p.mask[a] or (line is not None and (a in line) != (p.turn == color)):
                continue
            q = p.copy()
            R.step(q, a)
            found = go(q, acts + [a])
            if found:
                return found
        return None
    return go(R.reset("TicTacToe", 0), [])


def c4_game(rng, line, color):
    """A legal game whose last stone completes `line` for `color` (None: a draw): random play in which nobody makes
    a four but that one, the other color keeps off the line's cells, restarted until it works out."""
    while True:
        p = R.reset("ConnectFour", 0)
        acts = []
        while not p.done:
            safe, wanted = [], []
            for c in range(7):
                if not p.mask[c]:
                    continue
                cell = (5 - R.c4_filled(p.board, c)) * 7 + c
                on_line = line is not None and cell in line
                if on_line and p.turn != color:
                    continue
                b = list(p.board)
                b[cell] = p.turn
                if R.c4_won(b, p.turn):
                    if on_line and all(b[i] == color for i in line):
                        wanted = [c]
                        break
                    continue
                (wanted if on_line else safe).append(c)
            pick = wanted or safe
            if not pick:
                break
            a = int(pick[rng.integers(len(pick))])
            R.step(p, a)
            acts.append(a)
        if p.done:
            won = R.c4_won(p.board, 0) or R.c4_won(p.board, 1)
            if (line is None and not won) or (line is not None and won and all(p.board[i] == color for i in line)):
                return acts


def othello_games(rng):
    """Random games under mixed policies until the wanted endings and captures have all been seen: the games to
    play, each cut after what it is wanted for by an action of -1."""
    want = {"wipe": 2, "second_pass": 3, "tie": 2, "row6": 1, "col6": 1, "diag6": 1}
    games = []
    while any(v > 0 for v in want.values()):
        p = R.reset("Othello", 0)
        acts, cut = [], None
        greedy = int(rng.integers(0, 3))  # 0: both random; 1, 2: that side takes the most, the other the fewest
        while not p.done:
            legal = [a for a in range(65) if p.mask[a]]
            if greedy and legal != [64]:
                flips = [sum(len(R.othello_run(p.board, a, d)) for d in range(8)) for a in legal]
                best = max(flips) if p.turn == greedy - 1 else min(flips)
                legal = [a for a, f in zip(legal, flips) if f == best]
            a = int(legal[rng.integers(len(legal))])
            if a < 64 and cut is None:
                for d in range(8):
                    if len(R.othello_run(p.board, a, d)) == 6:
                        tag = "row6" if d < 2 else "col6" if d < 4 else "diag6"
                        if want[tag] > 0:
                            want[tag] -= 1
                            cut = len(acts) + 1
            mover_passed = p.passed
            rw = R.step(p, a)
            acts.append(a)
            if cut is not None:
                break
        if cut is not None:
            games.append(acts + ([] if p.done else [-1]))
            continue
        tag = "wipe" if 1 not in p.board and -1 in p.board and 0 in p.board else \
            "second_pass" if a == 64 and mover_passed else None
        keep = False
        if tag and want[tag] > 0:
            want[tag] -= 1
            keep = True
        if rw == [0.0, 0.0] and want["tie"] > 0:
            want["tie"] -= 1
            keep = True
        if keep:
            games.append(acts)
    # moves onto occupied cells: after a random opening, onto an own / opponent's cell from which a capture scan
    # succeeds / finds nothing
    for sign in (1, -1):
        for scans in (True, False):
            while True:
                p = R.reset("Othello", 0)
                acts = []
                for _ in range(int(rng.integers(6, 30))):
                    legal = [a for a in range(65) if p.mask[a]]
                    a = int(legal[rng.integers(len(legal))])
                    R.step(p, a)
                    acts.append(a)
                    if p.done:
                        break
                cells = [q for q in range(64) if p.board[q] == sign and
                         any(R.othello_run(p.board, q, d) for d in range(8)) == scans]
                if not p.done and cells:
                    games.append(acts + [int(cells[rng.integers(len(cells))])])
                    break
    return games


def hex_path():
    """A winding chain of 51 cells for color 0 (row 0 to row 10): rows 2, 4, 6, 8 in full, joined at alternating
    ends, in the order a walk along it meets them."""
    cells = [(0, 10), (1, 10)]
    for x in (2, 4, 6, 8):
        ys = range(10, -1, -1) if x % 4 == 2 else range(11)
        cells += [(x, y) for y in ys]
        cells.append((x + 1, 0 if x % 4 == 2 else 10))
    cells.append((10, 10))
    assert len(cells) == 51 and len(set(cells)) == 51
    return [x * 11 + y for x, y in cells]


def hex_games():
    games = []
    diagonal = [x * 12 for x in range(11)]
    firsts = diagonal + [10, 110] + [q for q in range(1, 120, 5) if q % 12 and q not in (10, 110)]
    assert len(set(firsts)) >= 30
    for q in firsts:
        games.append([q, 121, -1])
    path = hex_path()
    for color in (0, 1):
        chain = path if color == 0 else [(q % 11) * 11 + q // 11 for q in path]
        rest = [q for q in range(121) if q not in chain]
        acts = []
        for i, q in enumerate(chain):
            acts += [q, rest[i]] if color == 0 else [rest[i], q]
        p = R.reset("Hex", 0)
        for n, a in enumerate(acts):
            assert p.mask[a] and not p.done
            R.step(p, a)
            if p.done:
                acts = acts[:n + 1]
                break
        assert p.done and len(acts) >= 2 * 51 - 1
        games.append(acts)
    games.append([60, 61, 60])  # onto an own cell: the side to move placed 60 itself
    games.append([60, 61, 61])  # onto the opponent's cell
    return games


# --------------------------------------------------------------------------------------------------------------- scripts
def script(game, seed, n):
    rng = np.random.default_rng(20261020)
    if game == "TicTacToe":
        tasks = [("line", line, seat) for line in TTT_LINES for seat in (0, 1)] + [("draw", None, None)] * 3
    elif game == "ConnectFour":
        tasks = [("line", line, i % 2) for i, line in enumerate(c4_lines())] + [("draw", None, None)] * 3
        tasks += [("full", c, None) for c in range(7)]
    elif game == "Othello":
        tasks = [("game", g, None) for g in othello_games(rng)]
    else:
        tasks = [("game", g, None) for g in hex_games()]
    per_env = [[] for _ in range(n)]
    resets = [0] * n
    flips = [coins(seed, e, len(tasks) + 64) for e in range(n)]
    for kind, what, arg in tasks:
        e = min(range(n), key=lambda i: len(per_env[i]))
        coin = flips[e][resets[e]]
        if kind == "game":
            acts = what
        elif game == "TicTacToe":
            # the seat that moves first (the coin) holds color 0
            acts = ttt_game(what, None if kind == "draw" else (0 if coin == arg else 1))
        elif kind == "full":
            acts = [what] * 7
        else:
            acts = c4_game(rng, what, arg)
        per_env[e] += list(acts) + [0]  # the action after the end is ignored by the auto-reset
        resets[e] += 1
    steps = max(len(a) for a in per_env)
    out = np.zeros((steps, n), np.int32)
    for e in range(n):
        # fill up with the first legal action of whatever game is then being played
        p, k = R.reset(game, flips[e][0]), 0
        for t in range(steps):
            if t >= len(per_env[e]):
                per_env[e].append(next(a for a in range(R.A[game]) if p.mask[a]))
            a = per_env[e][t]
            if p.done:
                k += 1
                p = R.reset(game, flips[e][k])
            else:
                R.step(p, a)
            out[t, e] = a
    return out


# --------------------------------------------------------------------------------------------------------------- coverage
def coverage(game, g):
    """What the recorded run g shows: a dict of sets and counts."""
    cells = R.H[game] * R.W[game]
    acts, done, rew, hid = g["actions"], g["done"], g["reward"], g["hidden"]
    mask = g["info:legal_action_mask"]
    steps, n = acts.shape
    c = {"lines": set(), "colors": set(), "draws": 0, "full": set(), "wipe": 0, "second_pass": 0, "tie": 0,
         "run6": set(), "occupied": set(), "swaps": set(), "chains": set(), "placed_on": set()}
    lines4 = c4_lines()
    for t in range(steps):
        for e in range(n):
            if done[t, e]:
                continue
            a = int(acts[t, e])
            before = [int(np.sign(x)) if game == "Hex" else int(x) for x in hid[t, e, :cells]]
            after = [int(np.sign(x)) if game == "Hex" else int(x) for x in hid[t + 1, e, :cells]]
            turn = int(hid[t, e, cells])
            legal = 0 <= a < R.A[game] and bool(mask[t, e, a])
            over = bool(done[t + 1, e])
            r = [float(x) for x in rew[t + 1, e]]
            if game == "TicTacToe" and legal and over:
                if r == [0.0, 0.0]:
                    c["draws"] += 1
                else:
                    seat = r.index(1.0)
                    for line in TTT_LINES:
                        if a in line and all(after[i] == turn for i in line):
                            c["lines"].add((line, seat))
            elif game == "ConnectFour":
                if not legal and 0 <= a < 7:
                    c["full"].add(a)
                if legal and over:
                    if r == [0.0, 0.0]:
                        c["draws"] += 1
                    else:
                        c["colors"].add(turn)
                        cell = (5 - R.c4_filled(before, a)) * 7 + a
                        for line in lines4:
                            if cell in line and all(after[i] == turn for i in line):
                                c["lines"].add(line)
            elif game == "Othello":
                if 0 <= a < 64:
                    runs = [R.othello_run(before, a, d) for d in range(8)]
                    if legal:
                        for d in range(8):
                            if len(runs[d]) == 6:
                                c["run6"].add("row" if d < 2 else "col" if d < 4 else "diag")
                    elif before[a] != 0:
                        c["occupied"].add(("own" if before[a] > 0 else "opp", any(runs)))
                if legal and over:
                    if 1 not in after and 0 in after:  # after: from the next side's view, it has no stone left
                        c["wipe"] += 1
                    if a == 64:
                        c["second_pass"] += 1
                    if r == [0.0, 0.0]:
                        c["tie"] += 1
            elif game == "Hex":
                if legal and a == 121:
                    c["swaps"].add(next(i for i in range(121) if before[i] != 0))
                if 0 <= a < 121 and before[a] != 0:
                    c["placed_on"].add("own" if before[a] > 0 else "opp")
                if legal and over and len(R.hex_connected(after, a)) >= 30:
                    c["chains"].add(turn % 2)
    return c


def check(game, g):
    c = coverage(game, g)
    if game == "TicTacToe":
        assert c["lines"] == {(line, seat) for line in TTT_LINES for seat in (0, 1)} and c["draws"] >= 3, c
    elif game == "ConnectFour":
        assert c["lines"] == set(c4_lines()) and c["colors"] == {0, 1} and c["draws"] >= 3, c
        assert c["full"] == set(range(7)), c
    elif game == "Othello":
        assert c["wipe"] >= 2 and c["second_pass"] >= 3 and c["tie"] >= 2 and c["run6"] == {"row", "col", "diag"}, c
        assert c["occupied"] == {(k, s) for k in ("own", "opp") for s in (True, False)}, c
    else:
        diagonal = {x * 12 for x in range(11)}
        assert len(c["swaps"]) >= 30 and diagonal | {0, 10, 110, 120} <= c["swaps"], c
        assert c["chains"] == {0, 1} and c["placed_on"] == {"own", "opp"}, c
    return c
