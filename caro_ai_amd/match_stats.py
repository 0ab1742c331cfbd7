"""The statistics of an arena match, from net1's results ordered by uid (what lib.utils.play_games returns).

A match from paired openings (play_games(..., opening_pairs=True)) plays every opening twice with the colours swapped:
games 2j and 2j + 1 are one pair, and the pair, not the game, is the independent sample.  Its nine possible outcomes
are counted in a 3 x 3 table -- nine integers are all the ranks of a distributed match have to add up -- and every
figure below derives from the table.  An unpaired match has the per-game figures only.

CPU only; nothing here needs more than numpy."""
import math

import numpy as np

_Z95 = 1.96


def pair_table(results):
    """3 x 3 int64 table of a paired match: table[a + 1, b + 1] counts the pairs whose game 2j ended a and whose game
    2j + 1 ended b, for net1's results a, b in {-1, 0, +1}.  ValueError for an odd number of results or another value."""
    r = np.asarray(results, dtype=np.int64).reshape(-1)
    if len(r) & 1:
        raise ValueError("pair_table: a paired match has an even number of games, got %d" % len(r))
    if len(r) and (np.abs(r) > 1).any():
        raise ValueError("pair_table: results must be -1, 0 or +1")
    table = np.zeros((3, 3), dtype=np.int64)
    np.add.at(table, (r[0::2] + 1, r[1::2] + 1), 1)
    return table


def _elo(score):
    if score <= 0.0:
        return -math.inf
    if score >= 1.0:
        return math.inf
    return 400.0 * math.log10(score / (1.0 - score))


def _se(values, counts):
    """sample standard deviation (ddof = 1) of `values` taken `counts` times each, over the root of their number"""
    n = int(counts.sum())
    if n < 2:
        return 0.0
    mean = float((values * counts).sum()) / n
    var = float((counts * (values - mean) ** 2).sum()) / (n - 1)
    return math.sqrt(var / n)


def _finish(out, se):
    score = out["score"]
    out["elo"] = _elo(score)
    # (the interval's ends are clipped into the open interval, so they stay finite where the score itself is 0 or 1)
    eps = 1e-12
    out["elo_lo"] = _elo(min(max(score - _Z95 * se, eps), 1.0 - eps))
    out["elo_hi"] = _elo(min(max(score + _Z95 * se, eps), 1.0 - eps))
    return out


def _game_part(wins, losses, draws):
    games = wins + losses + draws
    out = {"games": games, "wins": wins, "losses": losses, "draws": draws,
           "ratio": wins / games if games else 0.0,
           "score": (wins + 0.5 * draws) / games if games else 0.0,
           "se_games": _se(np.array([1.0, 0.0, 0.5]), np.array([wins, losses, draws], dtype=np.int64))}
    return out


def summary_games(results):
    """The figures of an unpaired match: games, wins, losses, draws; ratio = wins / games (the promotion gate's number);
    score = (wins + draws / 2) / games; se_games, the sample standard deviation (ddof = 1) of the per-game scores over
    the root of their number; elo = 400 log10(score / (1 - score)), infinite at 0 and 1; elo_lo / elo_hi from
    score -+ 1.96 se_games, clipped into (0, 1)."""
    r = np.asarray(results, dtype=np.int64).reshape(-1)
    out = _game_part(int((r > 0).sum()), int((r < 0).sum()), int((r == 0).sum()))
    return _finish(out, out["se_games"])


def summary(table):
    """The figures of a paired match from its pair_table: those of summary_games, and pairs; se_pairs, the sample
    standard deviation (ddof = 1) of the pair means over the root of the number of pairs; split_pairs, the pairs whose
    two games were won by the same side of the opening (net1 won one and lost the other: the opening decided, the pair
    mean is 0.5).  elo_lo / elo_hi use se_pairs."""
    t = np.asarray(table, dtype=np.int64)
    if t.shape != (3, 3) or (t < 0).any():
        raise ValueError("summary: a 3 x 3 table of counts is expected")
    wins = int(t[2, :].sum() + t[:, 2].sum())
    losses = int(t[0, :].sum() + t[:, 0].sum())
    draws = int(t[1, :].sum() + t[:, 1].sum())
    out = _game_part(wins, losses, draws)
    score = np.array([0.0, 0.5, 1.0])
    means = (score[:, None] + score[None, :]) / 2.0
    out["pairs"] = int(t.sum())
    out["se_pairs"] = _se(means.reshape(-1), t.reshape(-1))
    out["split_pairs"] = int(t[0, 2] + t[2, 0])
    return _finish(out, out["se_pairs"])


def text(s):
    """One line for the CLIs"""
    def f(x):
        return "%+.0f" % x if math.isfinite(x) else ("+inf" if x > 0 else "-inf")
    if "pairs" in s:
        unit = "pairs=%d, split=%d, se_pairs=%.4f (se_games=%.4f)" % (s["pairs"], s["split_pairs"], s["se_pairs"],
                                                                     s["se_games"])
    else:
        unit = "games=%d, se_games=%.4f" % (s["games"], s["se_games"])
    return "match: score=%.4f, %s, elo=%s [%s, %s]" % (s["score"], unit, f(s["elo"]), f(s["elo_lo"]), f(s["elo_hi"]))
