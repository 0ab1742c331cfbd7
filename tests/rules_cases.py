"""Hand-built m,n,k / caro positions aimed at the bit masks of the win tests (test data generator; it decides nothing).

A case is (board, move, player): an int8 board of n*n cells in the oracle's layout (row-major, 0 / 1 stones, 2 empty),
an empty cell for the mover to play, and the mover.  Playing it puts a run of the mover's stones through the move
along one of the four directions.  The cases vary
  - where the run sits: against every board edge and in every corner, in all four directions, and across the
    64-bit word boundaries of the key (cells 63 / 64, 127 / 128, 191 / 192);
  - how long it is: k - 1, k and k + 1;
  - what ends it: an empty cell, an opponent stone or the board's edge on each side;
  - where the decisive run is: a run of k elsewhere on a line through the move, apart from the move;
  - how full the board is: empty around the run, a random background, or a full board but the move (a draw unless
    the move wins).
What the rule makes of each case is for the oracle to say; tests compare kernels with it."""
import numpy as np

DIRS = ((0, 1), (1, 0), (1, 1), (1, -1))  # row, column, diagonal, anti-diagonal
EMPTY = 2


def _on(n, r, c):
    return 0 <= r < n and 0 <= c < n


def _run(n, r0, c0, d, length):
    """the cells of a run of `length` from (r0, c0) along DIRS[d], and the cells just before / after it (None when
    off the board); None when the run leaves the board"""
    dr, dc = DIRS[d]
    cells = [(r0 + t * dr, c0 + t * dc) for t in range(length)]
    if not all(_on(n, r, c) for r, c in cells):
        return None
    before, after = (r0 - dr, c0 - dc), (r0 + length * dr, c0 + length * dc)
    return cells, (before if _on(n, *before) else None), (after if _on(n, *after) else None)


def _line(n, r, c, d):
    """every on-board cell of the line through (r, c) along DIRS[d], in order"""
    dr, dc = DIRS[d]
    while _on(n, r - dr, c - dc):
        r, c = r - dr, c - dc
    out = []
    while _on(n, r, c):
        out.append((r, c))
        r, c = r + dr, c + dc
    return out


def _touches_edge(n, cells, before, after):
    return before is None or after is None or any(r in (0, n - 1) or c in (0, n - 1) for r, c in cells)


def _board(n, rng, background):
    if background == 0.0:
        return np.full(n * n, EMPTY, np.int8)
    u = rng.random(n * n)
    return np.where(u < background, rng.integers(0, 2, n * n), EMPTY).astype(np.int8)


def _case(n, run, ends, t_move, player, rng, background=0.0):
    """board with the run (all but the move) and its two end cells set; `ends` = (before, after), each 'empty' or
    'opp' (ignored where the end is off the board)"""
    cells, before, after = run
    b = _board(n, rng, background)
    for end, e in ((before, ends[0]), (after, ends[1])):
        if end is not None:
            b[end[0] * n + end[1]] = 1 - player if e == "opp" else EMPTY
    for r, c in cells:
        b[r * n + c] = player
    mr, mc = cells[t_move]
    b[mr * n + mc] = EMPTY
    return b, mr * n + mc, player


def edge_cases(n, k, rng):
    """runs of k - 1, k, k + 1 in every direction at every edge / corner (and a few inside), each with open, blocked,
    half-blocked ends; the move at the run's first, last or an inner cell"""
    out = []
    ends_all = [("empty", "empty"), ("opp", "opp"), ("opp", "empty"), ("empty", "opp")]
    count = 0
    for d in range(4):
        for length in sorted({max(k - 1, 1), k, min(k + 1, n)}):
            starts = [(r, c) for r in range(n) for c in range(n)]
            runs = [x for x in (_run(n, r, c, d, length) for r, c in starts) if x is not None]
            edge = [x for x in runs if _touches_edge(n, *x)]
            inner = [x for x in runs if not _touches_edge(n, *x)]
            if inner:
                edge += [inner[i] for i in rng.choice(len(inner), size=min(2, len(inner)), replace=False)]
            for run in edge:
                ends = ends_all if length == k else [("empty", "empty"), ("opp", "opp")]
                seen = set()
                for e in ends:
                    key = tuple(x if end is not None else "edge" for x, end in zip(e, run[1:]))
                    if key in seen:
                        continue
                    seen.add(key)
                    t = (0, length - 1, length // 2)[count % 3]
                    player = count & 1
                    bg = 0.3 if count % 5 == 4 else 0.0
                    out.append(_case(n, run, e, t, player, rng, bg))
                    count += 1
    return out


def whole_line_cases(n, k, rng):
    """a run of k on a line through the move that does not hold the move (at least one cell apart), open or blocked
    at both ends: a win test that looks only at the run through the move differs here"""
    out = []
    for d in range(4):
        lines = {tuple(_line(n, r, c, d)) for r in range(n) for c in range(n)}
        lines = sorted((ln for ln in lines if len(ln) >= k + 2), key=len, reverse=True)[:3]
        for li, line in enumerate(lines):
            L = len(line)
            for s in sorted({0, L - k, (L - k) // 2}):
                for ends in (("empty", "empty"), ("opp", "opp")):
                    far = [m for m in range(L) if m < s - 1 or m > s + k]
                    if not far:
                        continue
                    m = far[int(rng.integers(len(far)))]
                    player = (li + s) & 1
                    b = np.full(n * n, EMPTY, np.int8)
                    for j in range(s, s + k):
                        b[line[j][0] * n + line[j][1]] = player
                    for j in (s - 1, s + k):
                        if 0 <= j < L:
                            b[line[j][0] * n + line[j][1]] = 1 - player if ends[0] == "opp" else EMPTY
                    out.append((b, line[m][0] * n + line[m][1], player))
    return out


def word_boundary_cases(n, k, rng):
    """runs of k - 1 and k that start, end or cross at a 64-bit word boundary of the key (cell 64 w opens a word)"""
    out = []
    for w in (64, 128, 192):
        if w >= n * n:
            break
        for cell in (w - 1, w):
            r, c = divmod(cell, n)
            for d in range(4):
                dr, dc = DIRS[d]
                for length in sorted({max(k - 1, 1), k}):
                    for t in range(length):
                        run = _run(n, r - t * dr, c - t * dc, d, length)
                        if run is None:
                            continue
                        for e in (("empty", "empty"), ("opp", "opp")):
                            tm = t if (t + len(out)) % 2 == 0 else (length - 1 - t)
                            out.append(_case(n, run, e, tm, len(out) & 1, rng))
    return out


def full_board_cases(n, k, rng):
    """one empty cell left; filling it makes a run of k through the move (blocked by the opponent on both ends where
    the board allows, else against the edge) and nothing else of the mover's on the four lines through it: a draw
    under the caro rule when both ends are blocked, a win under m,n,k"""
    out = []
    for d in range(4):
        runs = [x for x in (_run(n, r, c, d, k) for r in range(n) for c in range(n)) if x is not None]
        both = [x for x in runs if x[1] is not None and x[2] is not None]
        pick = (both[:1] + both[len(both) // 2:len(both) // 2 + 1]) if both else runs[:1]
        for run in pick:
            player = len(out) & 1
            cells, before, after = run
            b = rng.integers(0, 2, n * n).astype(np.int8)
            t = int(rng.integers(k))
            mr, mc = cells[t]
            for dd in range(4):
                for r, c in _line(n, mr, mc, dd):
                    b[r * n + c] = 1 - player
            for r, c in cells:
                b[r * n + c] = player
            b[mr * n + mc] = EMPTY
            out.append((b, mr * n + mc, player))
    return out


def hand_built_cases(n, k, seed=0):
    """every family above for one board; `seed` fixes the random choices"""
    rng = np.random.default_rng(1000 * n + k + 7919 * seed)
    return (edge_cases(n, k, rng) + whole_line_cases(n, k, rng) + word_boundary_cases(n, k, rng)
            + full_board_cases(n, k, rng))
