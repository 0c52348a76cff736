"""The PGX rules' second oracle: a scalar, cell-by-cell restatement of one reset-free step of TicTacToe,
ConnectFour, Hex and Othello and of every output key, written from the documented behaviour of
envpool_amd/csrc/pgx_env.hip.h.  Boards are lists of ints, walked one cell and one direction at a time: wins by
walking lines, Othello captures as a loop from the placed cell, Hex connection by breadth-first search over the six
neighbours.  No cell sets, no shifted words.

A position `Pos` holds what the fixtures record as hidden words:
  TicTacToe / ConnectFour  board[i] = the color on cell i or -1; turn = the color to move; cp = the seat to move
  Hex                      board[i] = +1 a stone of the color to move, -1 the other's, 0 empty; turn = step count;
                           cp = the seat that plays color 0
  Othello                  board[i] as Hex; turn; cp = the seat to move; passed
and the legal action mask the next step checks.

The quirks it keeps: an out-of-range or masked action ends the game with +1 for the other seat and -1 for the mover
(`illegal`), but an in-range one is played first -- a full ConnectFour column places nothing and still changes
turn, Hex places on any cell, an occupied Othello cell gets the mover's stone and stays the opponent's too, Hex's
swap moves the first stone in cell order whoever owns it; discount is written for the first player row only; the
mask is all ones after an end.

`replay` rolls a fixture through it (test_pgx_rules_host.py), which is what pins it to the reference.  The position
families of the rule tests are in pgx_rules_families.py.
"""
from collections import deque

import numpy as np

H = {"TicTacToe": 3, "ConnectFour": 6, "Hex": 11, "Othello": 8}
W = {"TicTacToe": 3, "ConnectFour": 7, "Hex": 11, "Othello": 8}
C = {"TicTacToe": 2, "ConnectFour": 2, "Hex": 4, "Othello": 2}
A = {"TicTacToe": 9, "ConnectFour": 7, "Hex": 122, "Othello": 65}
KEYS = ["info:env_id", "info:players.env_id", "elapsed_step", "done", "reward", "discount", "step_type", "trunc",
        "obs", "info:board", "info:current_player", "info:legal_action_mask", "info:players.id"]
DTYPES = dict(zip(KEYS, ["int32", "int32", "int32", "bool", "float32", "float32", "int32", "bool", "bool", "int32",
                         "int32", "bool", "int32"]))
TTT_LINES = [(0, 1, 2), (3, 4, 5), (6, 7, 8), (0, 3, 6), (1, 4, 7), (2, 5, 8), (0, 4, 8), (2, 4, 6)]
# Othello's eight directions as (row step, column step)
DIRS8 = [(0, 1), (0, -1), (1, 0), (-1, 0), (1, -1), (-1, 1), (1, 1), (-1, -1)]
# Hex's six neighbours of (x, y), cell x * 11 + y
HEX_NB = [(0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1)]


def hidden_words(game):
    return H[game] * W[game] + (3 if game == "Othello" else 2)


class Pos:
    __slots__ = ("game", "board", "turn", "cp", "passed", "mask", "done")

    def __init__(self, game, board, turn, cp, passed=0, mask=None, done=0):
        self.game, self.board, self.turn, self.cp, self.passed, self.done = game, list(board), turn, cp, passed, done
        self.mask = list(mask) if mask is not None else legal_mask(self)

    def copy(self):
        return Pos(self.game, self.board, self.turn, self.cp, self.passed, self.mask, self.done)

    def hidden(self):
        w = self.board + [self.turn, self.cp]
        return w + [self.passed] if self.game == "Othello" else w


def from_hidden(game, words):
    """The position of a row of hidden words; its mask is the one the last legal step left."""
    cells = H[game] * W[game]
    w = [int(x) for x in words]
    return Pos(game, w[:cells], w[cells], w[cells + 1], w[cells + 2] if game == "Othello" else 0)


def reset(game, coin):
    cells = H[game] * W[game]
    if game == "Othello":
        board = [0] * 64
        board[28] = board[35] = 1
        board[27] = board[36] = -1
        return Pos(game, board, 0, coin)
    return Pos(game, [0 if game == "Hex" else -1] * cells, 0, coin)


# ---------------------------------------------------------------------------------------------------------------
def c4_filled(board, col):
    return sum(1 for r in range(6) if board[r * 7 + col] >= 0)


def c4_won(board, color):
    """A four of `color` on some line: walked from every cell along down, right and the two diagonals."""
    for r in range(6):
        for c in range(7):
            if board[r * 7 + c] != color:
                continue
            for dr, dc in ((1, 0), (0, 1), (1, 1), (1, -1)):
                ok = True
                for k in range(1, 4):
                    rr, cc = r + dr * k, c + dc * k
                    if not (0 <= rr < 6 and 0 <= cc < 7) or board[rr * 7 + cc] != color:
                        ok = False
                        break
                if ok:
                    return True
    return False


def ttt_won(board, color):
    return any(all(board[i] == color for i in line) for line in TTT_LINES)


def othello_run(board, pos, d):
    """The cells captured from `pos` along direction d: the run of -1 cells that a +1 cell closes; [] if the run
    is closed by an empty cell or the edge."""
    dr, dc = DIRS8[d]
    r, c = pos // 8 + dr, pos % 8 + dc
    run = []
    while 0 <= r < 8 and 0 <= c < 8 and board[r * 8 + c] < 0:
        run.append(r * 8 + c)
        r, c = r + dr, c + dc
    if not (0 <= r < 8 and 0 <= c < 8) or board[r * 8 + c] <= 0:
        return []
    return run


def othello_legal(board):
    """The empty cells from which the side to move (+1) captures."""
    if 1 not in board:
        return [0] * 64  # nothing closes a run
    return [1 if board[p] == 0 and any(othello_run(board, p, d) for d in range(8)) else 0 for p in range(64)]


def hex_connected(board, start):
    """The cells of start's color (the sign of board[start]) joined to it through the six neighbours."""
    sign = board[start]
    seen = {start}
    todo = deque([start])
    while todo:
        p = todo.popleft()
        x, y = p // 11, p % 11
        for dx, dy in HEX_NB:
            nx, ny = x + dx, y + dy
            if 0 <= nx < 11 and 0 <= ny < 11:
                q = nx * 11 + ny
                if q not in seen and board[q] == sign:
                    seen.add(q)
                    todo.append(q)
    return seen


def legal_mask(p):
    g, b = p.game, p.board
    if g == "TicTacToe":
        return [1 if b[i] < 0 else 0 for i in range(9)]
    if g == "ConnectFour":
        return [1 if c4_filled(b, c) < 6 else 0 for c in range(7)]
    if g == "Hex":
        return [1 if b[i] == 0 else 0 for i in range(121)] + [1 if p.turn == 1 else 0]
    legal = othello_legal(b)
    return legal + [0 if any(legal) else 1]


def _illegal(loser):
    r = [1.0, 1.0]
    r[loser] = -1.0
    return r


def _winner_rewards(winner_color, p):
    """By color, then by seat: the seat to move now (p.cp) holds the color to move now (p.turn)."""
    if winner_color < 0:
        return [0.0, 0.0]
    by_color = [-1.0, -1.0]
    by_color[winner_color] = 1.0
    return by_color if p.cp == p.turn else [by_color[1], by_color[0]]


def hex_current(p):
    return p.cp if p.turn % 2 == 0 else 1 - p.cp


def step(p, act):
    """One step of a game that is not over: plays `act` on p and returns the two seats' rewards."""
    g = p.game
    in_range = 0 <= act < A[g]
    illegal = not in_range or not p.mask[act]
    rewards = [0.0, 0.0]
    b = p.board
    if g in ("TicTacToe", "ConnectFour"):
        loser = p.cp
        winner = -1
        if in_range:
            cell = act
            if g == "ConnectFour":
                r = 5 - c4_filled(b, act)
                cell = r * 7 + act if r >= 0 else -1
            if cell >= 0:
                b[cell] = p.turn
            won = ttt_won(b, p.turn) if g == "TicTacToe" else c4_won(b, p.turn)
            winner = p.turn if won else -1
            p.turn = 1 - p.turn
            p.cp = 1 - p.cp
        if not illegal:
            p.mask = legal_mask(p)
            full = all(v >= 0 for v in b) if g == "TicTacToe" else not any(p.mask)
            p.done = 1 if winner >= 0 or full else 0
            if p.done:
                rewards = _winner_rewards(winner, p)
    elif g == "Hex":
        loser = hex_current(p)
        if in_range:
            if act != 121:
                b[act] = 1
                group = hex_connected(b, act)
                # color 0 joins row 0 to row 10, color 1 joins column 0 to column 10
                if p.turn % 2 == 0:
                    ends = [any(q // 11 == 0 for q in group), any(q // 11 == 10 for q in group)]
                else:
                    ends = [any(q % 11 == 0 for q in group), any(q % 11 == 10 for q in group)]
                p.done = 1 if all(ends) else 0
            else:
                first = next((i for i in range(121) if b[i] != 0), -1)
                if first >= 0:
                    x, y = first // 11, first % 11
                    b[first] = 0
                    b[y * 11 + x] = 1
            p.turn += 1
            for i in range(121):
                b[i] = -b[i]
        if not illegal:
            p.mask = legal_mask(p)
            if p.done:
                loser_seat = hex_current(p)  # the color to move now has lost
                rewards[loser_seat] = -1.0
                rewards[1 - loser_seat] = 1.0
    else:
        loser = p.cp
        if in_range:
            mine = [v > 0 for v in b]
            theirs = [v < 0 for v in b]
            if act < 64:
                for d in range(8):
                    for q in othello_run(b, act, d):
                        mine[q], theirs[q] = True, False
                mine[act] = True
            nxt = [1 if theirs[i] else -1 if mine[i] else 0 for i in range(64)]
            empties = sum(1 for i in range(64) if not mine[i] and not theirs[i])
            mc, oc = sum(mine), sum(theirs)
            p.done = 1 if empties == 0 or oc == 0 or (p.passed and act == 64) else 0
            if p.done and mc != oc:
                rewards = [-1.0, -1.0]
                rewards[p.cp if mc > oc else 1 - p.cp] = 1.0
            p.board = nxt
            p.turn = 1 - p.turn
            p.cp = 1 - p.cp
            p.passed = 1 if act == 64 else 0
            p.mask = legal_mask(p)
    if illegal:
        p.done = 1
        rewards = _illegal(loser)
    if p.done:
        p.mask = [1] * A[g]
    return rewards


# ---------------------------------------------------------------------------------------------------------------
def row(p, rewards, env_id, elapsed, limit):
    """Every state key of one env after a reset or step, as plain nested lists in the fixtures' per-env shapes (obs
    [2, H, W, C] flat, as bytes of 0 / 1: numpy reads those far faster than nested lists)."""
    g = p.game
    h, w = H[g], W[g]
    cur = hex_current(p) if g == "Hex" else p.cp
    obs = []
    for seat in range(2):
        cells = []
        for v in p.board:
            if g in ("TicTacToe", "ConnectFour"):
                my_color = p.turn if seat == p.cp else 1 - p.turn
                cells.append([v == my_color, v == 1 - my_color])
            elif g == "Othello":
                rel = v if seat == cur else -v
                cells.append([rel > 0, rel < 0])
            else:
                rel = v if seat == cur else -v
                color = p.turn % 2 if seat == cur else 1 - p.turn % 2
                cells.append([rel > 0, rel < 0, color == 1, p.turn == 1])
        obs += [x for cell in cells for x in cell]
    done = bool(p.done)
    return {
        "info:env_id": env_id,
        "info:players.env_id": [env_id, env_id],
        "elapsed_step": elapsed,
        "done": done,
        "reward": list(rewards),
        "discount": [0.0 if done else 1.0, 0.0],
        "step_type": 0 if elapsed == 0 else 2 if done else 1,
        "trunc": done and elapsed >= limit,
        "obs": bytes(obs),
        "info:board": [p.board[r * w:(r + 1) * w] for r in range(h)],
        "info:current_player": cur,
        "info:legal_action_mask": list(p.mask),
        "info:players.id": [0, 1],
    }


def _stack(game, rows):
    out = {k: np.array([r[k] for r in rows], DTYPES[k]) for k in KEYS if k != "obs"}
    obs = np.frombuffer(b"".join(r["obs"] for r in rows), np.uint8)
    out["obs"] = (obs != 0).reshape(len(rows), 2, H[game], W[game], C[game])
    return {k: out[k] for k in KEYS}


def replay(game, g, hidden):
    """Rolls fixture g (hidden: its hidden words with Hex's labels as signs) through `step`.  Returns every key
    and the hidden words as [steps + 1, n, ...]; a reset row's coin is read from the fixture's own hidden words
    (it is the generator's), everything else is computed."""
    acts = g["actions"]
    steps, n = acts.shape
    limit = int(g["max_episode_steps"])
    cells = H[game] * W[game]
    rows = [[None] * n for _ in range(steps + 1)]
    hid = np.zeros((steps + 1, n, hidden_words(game)), np.int64)
    for e in range(n):
        p, cur = None, 0
        for t in range(steps + 1):
            rewards = [0.0, 0.0]
            if t == 0 or p.done:
                cur = 0
                p = reset(game, int(hidden[t, e, cells + 1]))
            else:
                cur += 1
                rewards = step(p, int(acts[t - 1, e]))
            rows[t][e] = row(p, rewards, e, cur, limit)
            hid[t, e] = p.hidden()
    flat = _stack(game, [r for rs in rows for r in rs])
    return {k: v.reshape(steps + 1, n, *v.shape[1:]) for k, v in flat.items()}, hid


def step_rows(game, hidden, elapsed, actions, limit):
    """One step from each row of hidden words (envs that are not over): every key as [n, ...] and the new hidden
    words [n, W]; env ids are the row numbers."""
    n = len(actions)
    rows, hid = [], np.zeros((n, hidden_words(game)), np.int64)
    before = {}  # rows of one position with several actions: its mask is worked out once
    for i in range(n):
        key = hidden[i].tobytes()
        if key not in before:
            before[key] = from_hidden(game, hidden[i])
        p = before[key].copy()
        rewards = step(p, int(actions[i]))
        rows.append(row(p, rewards, i, int(elapsed[i]) + 1, limit))
        hid[i] = p.hidden()
    return _stack(game, rows), hid
