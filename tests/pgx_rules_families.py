"""The position families of the PGX rule tests (test_pgx_rules_host.py on the CPU, test_gpu_pgx_rules.py on the
GPU): crafted positions at the places where cell-set code goes wrong, as rows of hidden words with one action each.
What a row must give comes from the scalar restatement (pgx_rules_ref.py), computed once per family and cached.

A family is {game, hidden [n, W], elapsed [n], actions [n], limit}.  Positions need not be reachable.  Every family
holds both values of current_player (crafted positions twice, random ones by draw) and elapsed counts above 0; one
family per game (TRUNC) has max_episode_steps = its largest elapsed count after the step, so that rows that end there
are truncated and the others are not.
"""
import functools

import numpy as np

import pgx_rules_ref as R

INT_MAX = 2**31 - 1
TRUNC = {"ttt_all": 5, "c4_true_lines": 9, "othello_endings": 7, "hex_swap": 4}


class _Rows:
    def __init__(self, game):
        self.game, self.hidden, self.actions = game, [], []

    def add(self, board, turn, actions, passed=0, cps=(0, 1)):
        for cp in cps:
            tail = [turn, cp, passed] if self.game == "Othello" else [turn, cp]
            for a in actions:
                self.hidden.append(list(board) + tail)
                self.actions.append(a)

    def done(self, name):
        n = len(self.actions)
        limit = TRUNC.get(name, INT_MAX)
        last = limit - 1 if name in TRUNC else 6
        # elapsed before the step: 1 ... last, so a TRUNC family's rows reach the limit or stop one short of it
        elapsed = np.array([last - (i // 2 % 2) if name in TRUNC else 1 + i % last for i in range(n)], np.int32)
        return {"game": self.game, "hidden": np.array(self.hidden, np.int32).reshape(n, R.hidden_words(self.game)),
                "elapsed": elapsed, "actions": np.array(self.actions, np.int32), "limit": limit}


# ----------------------------------------------------------------------------------------------------------- TicTacToe
def ttt_positions():
    """Every board reachable by legal play from the empty one, finished ones included: {board: turn}."""
    start = R.reset("TicTacToe", 0)
    seen = {tuple(start.board): (0, False)}
    todo = [start]
    while todo:
        p = todo.pop()
        for a in range(9):
            if not p.mask[a]:
                continue
            q = p.copy()
            R.step(q, a)
            key = tuple(q.board)
            if key not in seen:
                seen[key] = (q.turn, bool(q.done))
                if not q.done:
                    todo.append(q)
    return seen


def ttt_all():
    rows = _Rows("TicTacToe")
    pos = ttt_positions()
    assert len(pos) == 5478, len(pos)
    for board, (turn, over) in sorted(pos.items()):
        if not over:
            rows.add(board, turn, range(-1, 10))
    return rows.done("ttt_all")


# --------------------------------------------------------------------------------------------------------- ConnectFour
def c4_lines():
    """The 69 lines of four cells, by walking from every cell along right, down and the two diagonals."""
    lines = []
    for dr, dc in ((0, 1), (1, 0), (1, 1), (1, -1)):
        for r in range(6):
            for c in range(7):
                cells = [(r + dr * k, c + dc * k) for k in range(4)]
                if all(0 <= rr < 6 and 0 <= cc < 7 for rr, cc in cells):
                    lines.append(tuple(rr * 7 + cc for rr, cc in cells))
    assert len(lines) == 69 and len({frozenset(x) for x in lines}) == 69
    return lines


def _c4_landing(cells, last, color):
    """A board with `cells` minus `last` of `color` and the column under `last` filled so that a stone dropped
    there lands on it, without a four of either color; None if both fillings make one."""
    for phase in (0, 1):
        board = [-1] * 42
        for i in cells:
            if i != last:
                board[i] = color
        r, c = last // 7, last % 7
        for k, rr in enumerate(range(r + 1, 6)):
            if board[rr * 7 + c] < 0:
                board[rr * 7 + c] = (1 - color) if (k + phase) % 2 == 0 else color
        if not R.c4_won(board, 0) and not R.c4_won(board, 1):
            return board
    return None


def c4_true_lines():
    rows = _Rows("ConnectFour")
    for line in c4_lines():
        for color in (0, 1):
            for last in line:
                if line[1] - line[0] == 7 and last != line[0]:
                    continue  # a vertical line is completed by its top cell only: a stone lands on top
                board = _c4_landing(line, last, color)
                assert board is not None, (line, last)
                p = R.Pos("ConnectFour", board, color, 0)
                R.step(p, last % 7)
                assert p.done and p.board[last] == color, (line, last)
                rows.add(board, color, [last % 7])
    return rows.done("c4_true_lines")


def c4_false_lines():
    """The fours a shifted AND without column masks would see: cells i, i+s, i+2s, i+3s that are no line."""
    rows = _Rows("ConnectFour")
    real = {frozenset(x) for x in c4_lines()}
    count = landed = 0
    for s in (1, 6, 7, 8):
        for i in range(42 - 3 * s):
            cells = (i, i + s, i + 2 * s, i + 3 * s)
            if frozenset(cells) in real:
                continue
            count += 1
            for color in (0, 1):
                for last in cells:
                    board = _c4_landing(cells, last, color)
                    if board is None:
                        continue
                    # the game goes on, unless the stone makes a real four
                    p = R.Pos("ConnectFour", board, color, 0)
                    R.step(p, last % 7)
                    assert p.board[last] == color and bool(p.done) == R.c4_won(p.board, color), (cells, last)
                    landed += 1
                    rows.add(board, color, [last % 7])
    assert count == (39 - 24) + (24 - 12) + 0 + (18 - 12), count
    # every set, color and cell gives a row unless both fillings of the column make a four before the move
    assert landed >= count * 2 * 3, landed
    return rows.done("c4_false_lines")


def c4_last_cell():
    """Boards with one empty cell.  The full boards come from patterns without a four (colors in pairs of rows,
    alternating along a row: no run longer than 2 in any direction); a win on the 42nd stone from the same boards
    with three cells next to the empty one recolored.  The restatement sorts them; at least 8 of each are kept."""
    rows = _Rows("ConnectFour")
    draws = wins = 0
    for k in range(2):
        for off in range(2):
            for mirror in range(2):
                full = [(((r + off) // 2) + (6 - c if mirror else c) + k) % 2 for r in range(6) for c in range(7)]
                assert not R.c4_won(full, 0) and not R.c4_won(full, 1)
                for col in range(7):
                    # the three other cells of a line through the empty cell (0, col), as (row, column) steps
                    for recolor in (None, ((0, 1), (0, 2), (0, 3)), ((0, -1), (0, -2), (0, -3)),
                                    ((0, -1), (0, 1), (0, 2)), ((1, 0), (2, 0), (3, 0)), ((1, 1), (2, 2), (3, 3)),
                                    ((1, -1), (2, -2), (3, -3))):
                        board = list(full)
                        board[col] = -1
                        color = full[col]
                        if recolor is not None:
                            color = 1 - full[col]
                            if not all(0 <= col + dc < 7 for _, dc in recolor):
                                continue
                            for dr, dc in recolor:
                                board[dr * 7 + col + dc] = color
                        if R.c4_won(board, 0) or R.c4_won(board, 1):
                            continue
                        p = R.Pos("ConnectFour", board, color, 0)
                        rw = R.step(p, col)
                        assert p.done
                        if rw == [0.0, 0.0]:
                            draws += 1
                        else:
                            wins += 1
                        rows.add(board, color, [col])
    assert draws >= 8 and wins >= 8, (draws, wins)
    return rows.done("c4_last_cell")


def c4_random():
    rows = _Rows("ConnectFour")
    rng = np.random.default_rng(41)
    for _ in range(2048):
        board = [-1] * 42
        for c in range(7):
            for r in range(5, 5 - int(rng.integers(0, 7)), -1):
                board[r * 7 + c] = int(rng.integers(0, 2))
        rows.add(board, int(rng.integers(0, 2)), range(-1, 8), cps=(int(rng.integers(0, 2)),))
    return rows.done("c4_random")


# ------------------------------------------------------------------------------------------------------------- Othello
def _ray(p, d):
    """The cells from p (excluded) to the board edge along direction d."""
    dr, dc = R.DIRS8[d]
    r, c = p // 8 + dr, p % 8 + dc
    out = []
    while 0 <= r < 8 and 0 <= c < 8:
        out.append(r * 8 + c)
        r, c = r + dr, c + dc
    return out


def _bystander(p, line):
    """A cell off every line through p and off `line`, for an opposing stone that no move at p touches."""
    pr, pc = p // 8, p % 8
    for q in (0, 63, 7, 56, 9, 54, 14, 49, 18, 45, 21, 42):
        r, c = q // 8, q % 8
        if q not in line and r != pr and c != pc and abs(r - pr) != abs(c - pc):
            return q
    raise AssertionError(p)


def othello_rays():
    rows = _Rows("Othello")
    longest = 0
    for p in range(64):
        for d in range(8):
            ray = _ray(p, d)
            for run in range(1, len(ray) + 1):
                closings = ["own", "empty"] if run < len(ray) else ["edge"]
                if run > 6 and closings != ["edge"]:
                    continue
                for how in closings:
                    board = [0] * 64
                    for q in ray[:run]:
                        board[q] = -1
                    if how == "own":
                        board[ray[run]] = 1
                        longest = max(longest, run)
                    board[_bystander(p, ray)] = -1
                    rows.add(board, p % 2, [p])
    assert longest == 6
    return rows.done("othello_rays")


def othello_wraps():
    """A run that reaches column 0 or 7 with an own stone on the cell a shifted word would reach next: the next or
    previous row's far column.  It must not close the run."""
    rows = _Rows("Othello")
    count = 0
    for p in range(64):
        for d in range(8):
            dr, dc = R.DIRS8[d]
            ray = _ray(p, d)
            if dc == 0 or not ray or ray[-1] % 8 != (7 if dc > 0 else 0):
                continue
            wrap = ray[-1] + dr * 8 + dc
            if not 0 <= wrap < 64 or wrap == p:
                continue
            assert wrap % 8 == (0 if dc > 0 else 7)
            board = [0] * 64
            for q in ray:
                board[q] = -1
            board[wrap] = 1
            q = R.Pos("Othello", board, 0, 0)
            assert not q.mask[p] or any(R.othello_run(board, p, e) for e in range(8) if e != d)
            rows.add(board, 0, [p])
            count += 1
    assert count > 100, count
    return rows.done("othello_wraps")


def othello_endings():
    rows = _Rows("Othello")
    rng = np.random.default_rng(43)
    # the last empty cell filled (legal or not)
    for i in range(48):
        board = [int(x) for x in rng.choice([-1, 1], 64)]
        p = int(rng.integers(0, 64))
        board[p] = 0
        rows.add(board, i % 2, [p], passed=i // 2 % 2)
    # the mover captures the last opposing stone
    for p in range(64):
        for d in range(8):
            ray = _ray(p, d)
            for run in (1, min(6, len(ray) - 1)):
                if 1 <= run < len(ray):
                    board = [0] * 64
                    for q in ray[:run]:
                        board[q] = -1
                    board[ray[run]] = 1
                    chk = R.Pos("Othello", board, 0, 0)
                    R.step(chk, p)
                    assert chk.done and chk.board.count(1) == 0
                    rows.add(board, 0, [p])
    # passes: no move for either side (pass is legal; the second pass ends the game), and with moves (illegal)
    stuck = [0] * 64
    stuck[0], stuck[63] = 1, -1
    open_ = list(R.reset("Othello", 0).board)
    tie = [0] * 64
    tie[0] = tie[2] = 1
    tie[63] = tie[61] = -1
    ahead = list(tie)
    ahead[4] = 1
    for board in (stuck, open_, tie, ahead):
        for passed in (0, 1):
            rows.add(board, passed, [64], passed=passed)
    assert R.Pos("Othello", stuck, 0, 0).mask[64] and not R.Pos("Othello", open_, 0, 0).mask[64]
    # equal counts at the end: a full board after one capture (30 + 1 + 1 against 33 - 1), and a double pass
    full = [-1] * 64
    full[0] = 0
    for q in [2, 8, 9] + list(range(37, 64)):
        full[q] = 1
    chk = R.Pos("Othello", full, 0, 0)
    assert R.step(chk, 0) == [0.0, 0.0] and chk.done and chk.board.count(0) == 0
    rows.add(full, 0, [0])
    chk = R.Pos("Othello", tie, 0, 0, passed=1)
    assert R.step(chk, 64) == [0.0, 0.0] and chk.done
    return rows.done("othello_endings")


def othello_random():
    rows = _Rows("Othello")
    rng = np.random.default_rng(47)
    scanning = 0
    for i in range(1026):
        empty = (0.6, 0.3, 0.08)[i % 3]
        board = [int(x) for x in rng.choice([0, 1, -1], 64, p=[empty, (1 - empty) / 2, (1 - empty) / 2])]
        p = R.Pos("Othello", board, int(rng.integers(0, 2)), 0)
        scans = [any(R.othello_run(board, q, d) for d in range(8)) for q in range(64)]
        kinds = {"legal": [], "empty": [], "own": [], "opp": []}
        for q in rng.permutation(64):
            q = int(q)
            kind = ("legal" if p.mask[q] else "empty") if board[q] == 0 else "own" if board[q] > 0 else "opp"
            # occupied cells from which a capture scan succeeds come first
            kinds[kind].insert(0, q) if (board[q] != 0 and scans[q]) else kinds[kind].append(q)
        acts = [-1, 64, 65]
        for cells in kinds.values():
            acts += cells[:8]
        scanning += sum(1 for q in acts[3:] if board[q] != 0 and scans[q])
        rows.add(board, p.turn, acts, passed=int(rng.integers(0, 2)), cps=(int(rng.integers(0, 2)),))
    assert scanning > 1000, scanning
    return rows.done("othello_random")


# ----------------------------------------------------------------------------------------------------------------- Hex
def _t(cells):
    """Transposed cells: color 0 joins row 0 to row 10 (x), color 1 column 0 to column 10 (y)."""
    return [(q % 11) * 11 + q // 11 for q in cells]


def _hex_board(mine, theirs=()):
    board = [0] * 121
    for q in theirs:
        board[q] = -1
    for q in mine:
        board[q] = 1
    return board


def hex_random():
    rows = _Rows("Hex")
    rng = np.random.default_rng(53)
    for i in range(1024):
        n0, n1 = (int(x) for x in rng.integers(30, 61, 2))
        cells = [int(q) for q in rng.permutation(121)]
        own, opp, empty = cells[:n0], cells[n0:n0 + n1], cells[n0 + n1:]
        assert len(empty) >= 1
        acts = [-1, 121, 122] + empty[:4] + own[:2] + opp[:2]
        turn = 2 * int(rng.integers(1, 50)) + i % 2
        rows.add(_hex_board(own, opp), turn, acts, cps=(i // 2 % 2,))
    return rows.done("hex_random")


def hex_snake():
    """The chain for color 0: rows 0, 2, ..., 10 in full, joined at alternating ends by one cell of the odd rows."""
    cells = [x * 11 + y for x in range(0, 11, 2) for y in range(11)]
    cells += [x * 11 + (10 if x % 4 == 1 else 0) for x in range(1, 11, 2)]
    assert len(cells) == 71
    return cells


def _spans(cells, color):
    """Whether the stones `cells` hold a group from color's first edge to its other one."""
    board = _hex_board(cells)
    along = (lambda q: q // 11) if color == 0 else (lambda q: q % 11)
    return any(along(q) == 0 and any(along(r) == 10 for r in R.hex_connected(board, q)) for q in cells)


def hex_snakes():
    rows = _Rows("Hex")
    snake = hex_snake()
    rest = [q for q in range(121) if q not in snake]
    for color in (0, 1):
        chain = snake if color == 0 else _t(snake)
        others = rest if color == 0 else _t(rest)
        assert _spans(chain, color)
        # the cells without which the chain does not span: the last stone is one of these
        cuts = [q for q in chain if not _spans([r for r in chain if r != q], color)]
        assert len(cuts) >= 40, len(cuts)
        for j, last in enumerate(cuts):
            theirs = others if j % 2 else others[::3]
            whole = [q for q in chain if q != last]
            assert len(whole) >= 60
            board = _hex_board(whole, theirs)
            p = R.Pos("Hex", board, 10 + color, 0)
            R.step(p, last)
            assert p.done
            rows.add(board, 10 + color, [last])
            # one stone short: a second cut cell is missing too
            gap = cuts[(j + 17) % len(cuts)]
            board = _hex_board([q for q in whole if q != gap], theirs)
            p = R.Pos("Hex", board, 10 + color, 0)
            R.step(p, last)
            assert not p.done, (color, last, gap)
            rows.add(board, 10 + color, [last])
    return rows.done("hex_snakes")


def hex_near_misses():
    """Lines broken at a step to (x + 1, y + 1), which is no neighbour, and groups that meet only where the end
    of one row and the start of the next are next to each other in cell order.  None of them connects.
    The cells (x, y) and (x + 1, y + 1) are each other's (x + 1, y + 1) and (x - 1, y - 1): the last stone is placed
    on either side of the break, so the fill starts once from the cell whose missing neighbour is (x + 1, y + 1)
    and once from the one whose is (x - 1, y - 1).  The row-end groups -- (x, 6..10) with (x + 1, 0..3), whose cells
    (x, 10) and (x + 1, 0) differ by one in cell order, the step a shifted word takes -- are placed as they are for
    both colors (only color 1, which joins column 0 to column 10, could win through such a wrap) and transposed for
    both (column-end groups: no shift joins them, a control)."""
    rows = _Rows("Hex")
    for color in (0, 1):
        for k in range(10):
            for y in (0, 4, 9):
                line = [x * 11 + (y if x <= k else y + 1) for x in range(11)]
                chain = line if color == 0 else _t(line)
                for last in (chain[k], chain[k + 1], chain[0], chain[10]):
                    board = _hex_board([q for q in chain if q != last])
                    p = R.Pos("Hex", board, 20 + color, 0)
                    R.step(p, last)
                    assert not p.done
                    rows.add(board, 20 + color, [last])
        for x in range(10):
            wrap = [x * 11 + y for y in range(6, 11)] + [(x + 1) * 11 + y for y in range(0, 4)]
            for group in (wrap, _t(wrap)):
                for last in (group[0], group[4], group[5], group[8]):
                    board = _hex_board([q for q in group if q != last])
                    p = R.Pos("Hex", board, 20 + color, 0)
                    R.step(p, last)
                    assert not p.done
                    rows.add(board, 20 + color, [last])
    return rows.done("hex_near_misses")


def hex_swap():
    rows = _Rows("Hex")
    for q in range(121):
        rows.add(_hex_board([], [q]), 1, [121])
    for q in (0, 5, 17, 120):  # a first stone of the side to move (no position of play)
        rows.add(_hex_board([q]), 1, [121])
    rows.add(_hex_board([]), 0, [121])
    for turn in (2, 3):
        for own, opp in (([3], [40]), ([40], [3]), ([100, 7], [55]), ([60], [60 + 11, 13])):
            rows.add(_hex_board(own, opp[:turn - 1]), turn, [121])
    return rows.done("hex_swap")


FAMILIES = {
    "ttt_all": ttt_all,
    "c4_true_lines": c4_true_lines, "c4_false_lines": c4_false_lines, "c4_last_cell": c4_last_cell,
    "c4_random": c4_random,
    "othello_rays": othello_rays, "othello_wraps": othello_wraps, "othello_endings": othello_endings,
    "othello_random": othello_random,
    "hex_swap": hex_swap, "hex_near_misses": hex_near_misses, "hex_snakes": hex_snakes, "hex_random": hex_random,
}

@functools.lru_cache(maxsize=None)
def family(name):
    """The family's rows and what the restatement says they give: (rows, keys, hidden)."""
    fam = FAMILIES[name]()
    want, hid = R.step_rows(fam["game"], fam["hidden"], fam["elapsed"], fam["actions"], fam["limit"])
    if name in TRUNC:
        over = want["done"]
        assert want["trunc"].any() and (over & ~want["trunc"]).any(), name
    assert set(fam["hidden"][:, R.H[fam["game"]] * R.W[fam["game"]] + 1]) == {0, 1}, name
    assert (fam["elapsed"] > 0).all() and set(want["step_type"]) <= {1, 2}, name
    return fam, want, hid


def differences(name, got, got_hidden):
    """The keys (or "hidden") in which `got` differs from the restatement, with the first row that does."""
    fam, want, hid = family(name)
    out = []
    for k in R.KEYS:
        g = np.asarray(got[k]).reshape(want[k].shape)
        if not np.array_equal(g, want[k]):
            bad = np.nonzero((g != want[k]).reshape(len(g), -1).any(1))[0]
            out.append((k, int(bad[0]), len(bad)))
    if not np.array_equal(np.asarray(got_hidden, np.int64), hid):
        bad = np.nonzero((np.asarray(got_hidden, np.int64) != hid).any(1))[0]
        out.append(("hidden", int(bad[0]), len(bad)))
    return out
