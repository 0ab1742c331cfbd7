"""The slot-row launch form of the net (include/caro_hip.h, "slot rows") restated in plain numpy, and the tile-class rule
of the row-Winograd kernel (csrc/caro_net_kernels.inc, k_net_forward_w) as a function of the launch size.

The rule of the header: game g keeps its j-th leaf at row g * B + j; gpack[g] = leaf count | net class << 8; a launch
serves the leaves of a class in GAME order (game 0's leaves first, each game's in row order), so dense board i of class c
is the i-th entry of game_order_rows(cnt, cls, B, c).  Nothing here shares code or method with the kernels' prefix sums:
the tests compare a slot launch with a dense launch of the rows listed here.
"""
import numpy as np

NT = 512      # threads of a net workgroup: the kernels give each thread ceil(G / NT) games of the count vector
GP_PRE = 4    # games per thread the row-Winograd kernels keep in registers; more take the plain map
CLASSES = ("4-way", "2-way", "full", "full+4-way", "full+2-way")


def game_order_rows(cnt, cls, B, c):
    """slot rows g * B + j of the leaves of class c, in game order"""
    return np.array([g * B + j for g in range(len(cnt)) if cls[g] == c for j in range(int(cnt[g]))], np.int64)


def gpack(cnt, cls):
    cnt, cls = np.asarray(cnt), np.asarray(cls)
    assert ((cnt >= 0) & (cnt <= 255)).all() and ((cls == 0) | (cls == 1)).all()
    return (cnt | (cls << 8)).astype(np.int32)


def totals(cnt, cls):
    cnt, cls = np.asarray(cnt), np.asarray(cls)
    return [int(cnt[cls == 0].sum()), int(cnt[cls == 1].sum())]


def slot_list(cnt, cls, B, rng):
    """i32[2][G * B]: row c lists the slot rows of class c in a shuffled order, -1 behind them"""
    out = np.full((2, len(cnt) * B), -1, np.int32)
    for c in (0, 1):
        rows = game_order_rows(cnt, cls, B, c)
        out[c, :len(rows)] = rng.permutation(rows)
    return out


def games_per_thread(G):
    return -(-G // NT)


def counts_with_total(G, B, L, seed, lead_empty=0, tail_empty=0, full_games=0):
    """int64[G] leaf counts in [0, B] with sum exactly L, the first lead_empty and the last tail_empty games at 0 and at
    least full_games games at exactly B; the same seed gives the same counts"""
    live = G - lead_empty - tail_empty
    assert live >= 0 and 0 <= full_games <= live and full_games * B <= L <= live * B, (G, B, L, lead_empty, tail_empty)
    rng = np.random.default_rng(seed)
    cnt = np.zeros(G, np.int64)
    idx = lead_empty + rng.permutation(live)
    fixed, free = idx[:full_games], idx[full_games:]
    cnt[fixed] = B
    rest = L - full_games * B
    assert rest <= len(free) * B
    if len(free):
        c = rng.integers(0, B + 1, len(free))
        while c.sum() != rest:  # move towards the total one leaf per game at a time: stays in [0, B]
            d = rest - int(c.sum())
            can = np.flatnonzero(c < B) if d > 0 else np.flatnonzero(c > 0)
            pick = rng.permutation(can)[:abs(d)]
            c[pick] += 1 if d > 0 else -1
        cnt[free] = c
    assert cnt.sum() == L and cnt.min(initial=0) >= 0 and cnt.max(initial=0) <= B
    assert not cnt[:lead_empty].any() and not cnt[G - tail_empty:].any()
    assert int((cnt == B).sum()) >= full_games
    return cnt


def split_tile_sizes(H, W, TB):
    """(TB2, TB4): boards of a 2-way / 4-way K-split tile of the row-Winograd kernel, 0 where the board has none.
    A board is ceil(H / 2) * W row tiles; a 2-way tile holds 64 of them, a 4-way tile 32.  A split tile that would be
    no smaller than the full tile does not exist, nor one whose activation rows (boards * H * W) would reach the rows
    the waves exchange their partial sums through (from row 127 / row 63)."""
    tpb = -(-H // 2) * W
    tb2, tb4 = 64 // tpb, 32 // tpb
    if tb2 >= TB or tb2 * H * W > 127:
        tb2 = 0
    if tb4 >= TB or tb4 * H * W > 63:
        tb4 = 0
    return tb2, tb4


def tile_class(L, TB, TB2, TB4, ncu, pair=False):
    """which tiles a row-Winograd launch of L boards runs (pair: L = L0 + L1 of a two-net launch).
    One net: every tile 4-way while L <= ncu * TB4, every tile 2-way while L <= ncu * TB2, otherwise full tiles of TB
    boards -- and when L exceeds one round of them (ncu * TB) by no more than ncu * TB4 / ncu * TB2, the first ncu
    tiles are full and the excess runs in 4-way / 2-way tiles.  Two nets: the same two small classes with ncu - 1 in
    place of ncu (each net's rows round up to whole tiles), and no overflow classes."""
    if pair:
        if ncu > 1 and TB4 > 0 and L <= (ncu - 1) * TB4:
            return "4-way"
        if ncu > 1 and TB2 > 0 and L <= (ncu - 1) * TB2:
            return "2-way"
        return "full"
    if ncu <= 0:
        return "full"
    if TB4 > 0 and L <= ncu * TB4:
        return "4-way"
    if TB2 > 0 and L <= ncu * TB2:
        return "2-way"
    over = L - ncu * TB
    if over > 0 and TB4 > 0 and over <= ncu * TB4:
        return "full+4-way"
    if over > 0 and TB2 > 0 and over <= ncu * TB2:
        return "full+2-way"
    return "full"


def _edges(TB, TB2, TB4, ncu, pair):
    """every L at which the class can change, and its successor"""
    n = ncu - 1 if pair else ncu
    e = {1, n * TB4, n * TB2}
    if not pair:
        e |= {ncu * TB, ncu * TB + ncu * TB4, ncu * TB + ncu * TB2}
    return sorted({x + d for x in e for d in (0, 1) if x + d >= 1})


def pad_to_class(n, c, TB, TB2, TB4, ncu, pair=False):
    """the smallest L >= n whose launch is of tile class c (None: there is none)"""
    for L in sorted({max(n, 1)} | {x for x in _edges(TB, TB2, TB4, ncu, pair) if x >= n}):
        if tile_class(L, TB, TB2, TB4, ncu, pair) == c:
            return L
    return None


def largest_of_class(c, TB, TB2, TB4, ncu, pair=False):
    """the largest L of the first run of launch sizes of class c (None: the class does not occur or has no end)"""
    lo = pad_to_class(1, c, TB, TB2, TB4, ncu, pair)
    if lo is None:
        return None
    for L in _edges(TB, TB2, TB4, ncu, pair):
        if L > lo and tile_class(L, TB, TB2, TB4, ncu, pair) != c:
            return L - 1
    return None


def boards_per_tile(c, TB, TB2, TB4):
    """boards of the tiles of class c: (the first round's, the overflow's or None)"""
    return {"4-way": (TB4, None), "2-way": (TB2, None), "full": (TB, None), "full+4-way": (TB, TB4),
            "full+2-way": (TB, TB2)}[c]
