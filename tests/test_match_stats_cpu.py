"""caro_ai_amd.match_stats on hand-written result lists, against the formulas written out with numpy here."""
import math

import numpy as np
import pytest

from caro_ai_amd import match_stats

CASES = {
    "all_wins": [1] * 8,
    "all_split": [1, -1, -1, 1, 1, -1, 1, -1],
    "mixed_with_draws": [1, 0, -1, -1, 0, 0, 1, 1, -1, 1, 0, -1, 1, -1],
    "single_pair": [1, 0],
}


def _elo(p):
    return -math.inf if p <= 0 else math.inf if p >= 1 else 400.0 * math.log10(p / (1.0 - p))


def _clip(p):
    return min(max(p, 1e-12), 1.0 - 1e-12)


def _want(results):
    r = np.asarray(results)
    per_game = (r + 1) / 2.0
    pair_mean = (per_game[0::2] + per_game[1::2]) / 2.0
    n, m = len(r), len(r) // 2
    se_games = per_game.std(ddof=1) / math.sqrt(n) if n > 1 else 0.0
    se_pairs = pair_mean.std(ddof=1) / math.sqrt(m) if m > 1 else 0.0
    score = per_game.mean()
    return {"games": n, "wins": int((r == 1).sum()), "losses": int((r == -1).sum()), "draws": int((r == 0).sum()),
            "ratio": (r == 1).sum() / n, "score": score, "se_games": se_games, "pairs": m, "se_pairs": se_pairs,
            "split_pairs": int((r[0::2] * r[1::2] == -1).sum()), "elo": _elo(score),
            "elo_lo": _elo(_clip(score - 1.96 * se_pairs)), "elo_hi": _elo(_clip(score + 1.96 * se_pairs))}


def _close(got, want, key):
    if isinstance(want, float) and math.isinf(want):
        assert got == want, key
    else:
        assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (key, got, want)


@pytest.mark.parametrize("name", list(CASES))
def test_pair_table_and_summary_equal_the_formulas(name):
    results = CASES[name]
    table = match_stats.pair_table(results)
    assert table.shape == (3, 3) and table.dtype == np.int64 and int(table.sum()) == len(results) // 2
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            assert table[a + 1, b + 1] == sum(1 for x, y in zip(results[0::2], results[1::2]) if (x, y) == (a, b))
    got, want = match_stats.summary(table), _want(results)
    assert set(got) == set(want)
    for k, w in want.items():
        _close(got[k], w, k)
    # the unpaired summary of the same games: the per-game figures, the interval from se_games
    flat = match_stats.summary_games(results)
    assert not {"pairs", "se_pairs", "split_pairs"} & set(flat)
    for k in ("games", "wins", "losses", "draws", "ratio", "score", "se_games", "elo"):
        _close(flat[k], want[k], k)
    _close(flat["elo_lo"], _elo(_clip(want["score"] - 1.96 * want["se_games"])), "elo_lo")
    _close(flat["elo_hi"], _elo(_clip(want["score"] + 1.96 * want["se_games"])), "elo_hi")
    # the tables of two halves of a match add up to the table of the whole: what the ranks all-reduce
    if len(results) >= 4:
        cut = 2 * (len(results) // 4)
        assert (match_stats.pair_table(results[:cut]) + match_stats.pair_table(results[cut:]) == table).all()


def test_split_pairs_have_no_pair_error_but_a_game_error():
    s = match_stats.summary(match_stats.pair_table(CASES["all_split"]))
    assert s["se_pairs"] == 0.0 and s["se_games"] > 0.25 / math.sqrt(8) and s["split_pairs"] == s["pairs"] == 4
    assert s["score"] == 0.5 and s["elo"] == 0.0 and s["elo_lo"] == s["elo_hi"] == 0.0


def test_elo_is_infinite_at_the_ends():
    win = match_stats.summary(match_stats.pair_table([1] * 8))
    loss = match_stats.summary(match_stats.pair_table([-1] * 8))
    assert win["score"] == 1.0 and win["elo"] == math.inf and win["ratio"] == 1.0
    assert loss["score"] == 0.0 and loss["elo"] == -math.inf and loss["ratio"] == 0.0
    assert math.isfinite(win["elo_lo"]) and math.isfinite(loss["elo_hi"])
    assert match_stats.summary_games([1, 1, 1])["elo"] == math.inf
    for s in (win, loss, match_stats.summary(match_stats.pair_table(CASES["mixed_with_draws"]))):
        line = match_stats.text(s)
        assert line.startswith("match: score=%.4f, pairs=%d, " % (s["score"], s["pairs"])) and "\n" not in line


def test_bad_input_is_refused():
    with pytest.raises(ValueError):
        match_stats.pair_table([1, -1, 0])
    with pytest.raises(ValueError):
        match_stats.pair_table([1, 2])
    with pytest.raises(ValueError):
        match_stats.summary(np.zeros((2, 3), np.int64))
    assert int(match_stats.pair_table([]).sum()) == 0
