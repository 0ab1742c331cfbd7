"""tests/slot_rows.py -- the numpy statement of the slot-row map and of the net's tile classes that
tests/test_gpu_net_launch_forms.py compares the kernels with -- on cases worked out by hand.  No GPU."""
import numpy as np
import pytest

from tests import slot_rows as sr

C4 = dict(TB=6, TB2=3, TB4=1, ncu=256)  # connect four on a 256-unit device: 21 row tiles per board


def test_three_games_by_hand():
    """B = 4, counts (2, 0, 3): game 0 owns rows 0..3 and uses 0, 1; game 1 none; game 2 owns 8..11 and uses 8, 9, 10"""
    cnt, cls = np.array([2, 0, 3]), np.array([0, 0, 0])
    assert sr.game_order_rows(cnt, cls, 4, 0).tolist() == [0, 1, 8, 9, 10]
    assert sr.game_order_rows(cnt, cls, 4, 1).tolist() == []
    assert sr.gpack(cnt, cls).tolist() == [2, 0, 3] and sr.gpack(cnt, cls).dtype == np.int32
    assert sr.totals(cnt, cls) == [5, 0]


def test_two_classes_by_hand():
    """B = 3, counts (1, 3, 0, 2), classes (1, 0, 1, 1): class 0 is game 1 alone (rows 3, 4, 5); class 1 is game 0
    (row 0), game 2 (nothing) and game 3 (rows 9, 10)"""
    cnt, cls = np.array([1, 3, 0, 2]), np.array([1, 0, 1, 1])
    assert sr.game_order_rows(cnt, cls, 3, 0).tolist() == [3, 4, 5]
    assert sr.game_order_rows(cnt, cls, 3, 1).tolist() == [0, 9, 10]
    assert sr.gpack(cnt, cls).tolist() == [1 | 256, 3, 256, 2 | 256]
    assert sr.totals(cnt, cls) == [3, 3]
    sl = sr.slot_list(cnt, cls, 3, np.random.default_rng(0))
    assert sl.shape == (2, 12) and sl.dtype == np.int32
    assert sorted(sl[0, :3].tolist()) == [3, 4, 5] and (sl[0, 3:] == -1).all()
    assert sorted(sl[1, :3].tolist()) == [0, 9, 10] and (sl[1, 3:] == -1).all()


def test_slot_list_shuffles():
    cnt, cls = np.full(40, 5), np.arange(40) % 2
    sl = sr.slot_list(cnt, cls, 8, np.random.default_rng(1))
    for c in (0, 1):
        rows = sr.game_order_rows(cnt, cls, 8, c)
        assert len(rows) == 100 and sorted(sl[c, :100].tolist()) == rows.tolist()
        assert sl[c, :100].tolist() != rows.tolist()


def test_gpack_holds_the_whole_count_field():
    assert sr.gpack([255, 0], [1, 1]).tolist() == [255 | 256, 256]
    with pytest.raises(AssertionError):
        sr.gpack([256], [0])


def test_games_per_thread():
    assert [sr.games_per_thread(g) for g in (1, 512, 513, 1024, 1025, 2048, 2049, 4096)] == [1, 1, 2, 2, 3, 4, 5, 8]
    assert sr.games_per_thread(2048) <= sr.GP_PRE < sr.games_per_thread(2049)


def test_counts_with_total_keeps_its_promises():
    rng = np.random.default_rng(7)
    for seed in range(300):
        G = int(rng.integers(1, 60))
        B = int(rng.integers(1, 12))
        lead = int(rng.integers(0, G + 1)) if seed % 3 == 0 else 0
        tail = int(rng.integers(0, G - lead + 1)) if seed % 4 == 0 else 0
        live = G - lead - tail
        full = int(rng.integers(0, live + 1)) if seed % 5 == 0 else 0
        L = int(rng.integers(full * B, live * B + 1))
        cnt = sr.counts_with_total(G, B, L, seed, lead, tail, full)
        assert cnt.shape == (G,) and cnt.sum() == L and cnt.min() >= 0 and cnt.max() <= B
        assert not cnt[:lead].any() and not cnt[G - tail:].any()
        assert (cnt == B).sum() >= full
        assert np.array_equal(cnt, sr.counts_with_total(G, B, L, seed, lead, tail, full))
    assert sr.counts_with_total(1, 1, 0, 0).tolist() == [0]
    assert sr.counts_with_total(3, 4, 12, 0).tolist() == [4, 4, 4]
    assert sr.counts_with_total(5, 2, 4, 0, lead_empty=3).tolist() == [0, 0, 0, 2, 2]
    with pytest.raises(AssertionError):
        sr.counts_with_total(4, 2, 9, 0)
    with pytest.raises(AssertionError):
        sr.counts_with_total(4, 2, 5, 0, lead_empty=1, tail_empty=1)


def test_split_tile_sizes():
    assert sr.split_tile_sizes(6, 7, 6) == (3, 1)      # 21 row tiles per board: 64 // 21, 32 // 21
    assert sr.split_tile_sizes(3, 3, 21) == (10, 5)    # 6 per board
    assert sr.split_tile_sizes(5, 5, 8) == (4, 2)      # 15 per board
    assert sr.split_tile_sizes(8, 8, 3) == (0, 0)      # 2 boards = 128 rows / 1 board = 64 rows reach the exchange rows
    assert sr.split_tile_sizes(4, 4, 15) == (0, 0)     # likewise 8 boards = 128 rows / 4 boards = 64 rows
    assert sr.split_tile_sizes(6, 6, 7) == (3, 1)      # 108 and 36 rows stay below rows 127 / 63
    assert sr.split_tile_sizes(3, 3, 10) == (0, 5)     # a 2-way tile no smaller than the full tile does not exist
    assert sr.split_tile_sizes(3, 3, 5) == (0, 0)
    assert sr.split_tile_sizes(15, 15, 1) == (0, 0)    # one board fills the tile


@pytest.mark.parametrize("L,want", [(1, "4-way"), (255, "4-way"), (256, "4-way"), (257, "2-way"), (768, "2-way"),
                                    (769, "full"), (1536, "full"), (1537, "full+4-way"), (1792, "full+4-way"),
                                    (1793, "full+2-way"), (2304, "full+2-way"), (2305, "full"), (3100, "full")])
def test_tile_class_of_connect_four(L, want):
    assert sr.tile_class(L, **C4) == want


@pytest.mark.parametrize("L,want", [(255, "4-way"), (256, "2-way"), (765, "2-way"), (766, "full"), (1700, "full"),
                                    (2000, "full")])
def test_tile_class_of_a_connect_four_pair(L, want):
    assert sr.tile_class(L, pair=True, **C4) == want


def test_tile_class_without_split_tiles():
    assert sr.tile_class(10, 6, 0, 0, 256) == "full" and sr.tile_class(5000, 6, 0, 0, 256) == "full"
    assert sr.tile_class(10, 6, 3, 1, 0) == "full"                    # split tiles switched off
    assert sr.tile_class(300, 3, 0, 1, 256) == "full"                 # a board with 4-way tiles only
    assert sr.tile_class(256 * 3 + 256, 3, 0, 1, 256) == "full+4-way"
    assert sr.tile_class(256 * 3 + 257, 3, 0, 1, 256) == "full"


def test_class_ranges():
    assert sr.pad_to_class(100, "4-way", **C4) == 100
    assert sr.pad_to_class(100, "2-way", **C4) == 257
    assert sr.pad_to_class(100, "full", **C4) == 769
    assert sr.pad_to_class(1690, "full", **C4) == 2305
    assert sr.pad_to_class(1000, "full", **C4) == 1000
    assert sr.pad_to_class(1, "full+2-way", **C4) == 1793
    assert sr.pad_to_class(300, "4-way", **C4) is None
    assert [sr.largest_of_class(c, **C4) for c in sr.CLASSES] == [256, 768, 1536, 1792, 2304]
    five = dict(TB=8, TB2=4, TB4=2, ncu=256)
    assert [sr.largest_of_class(c, **five) for c in sr.CLASSES] == [512, 1024, 2048, 2560, 3072]
    assert sr.largest_of_class("2-way", pair=True, **five) == 1020
    assert sr.boards_per_tile("full+4-way", 6, 3, 1) == (6, 1) and sr.boards_per_tile("2-way", 6, 3, 1) == (3, None)
