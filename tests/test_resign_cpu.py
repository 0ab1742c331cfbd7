"""Resignation on the CPU: the playthrough uniform of caro_noise.h (host export) against a plain-Python statement, and
the host bookkeeping of caro_ai_amd/resign.py (split_games, false_positive_rate, calibrate) on hand-built games whose
answers are worked out below."""
import math

import numpy as np
import pytest

from tests.synth_net import MASK, _mix64_py


def _L():
    from caro_ai_amd import _lib
    return _lib.load()


def _resign_uniform_py(seed, uid):
    """caro_resign_uniform: mix64(mix64(seed ^ "resig") + uid), 52 bits -> (0, 1)"""
    k = _mix64_py(seed ^ 0x7265736967)
    k = _mix64_py((k + uid) & MASK)
    return ((k >> 12) + 0.5) * (1.0 / 4503599627370496.0)


def test_resign_uniform_is_its_python_statement():
    L = _L()
    rng = np.random.default_rng(3)
    seeds = [0, 1, 7, 2 ** 64 - 1, int(rng.integers(0, 2 ** 63))]
    uids = list(range(2000)) + [int(u) for u in rng.integers(0, 2 ** 63, 8000, dtype=np.int64)]
    for i, uid in enumerate(uids):
        seed = seeds[i % len(seeds)]
        assert L.caro_host_resign_uniform(seed, uid) == _resign_uniform_py(seed, uid), (seed, uid)
    # its own stream: not the move uniform of ply 0 nor of any other small ply
    assert all(L.caro_host_resign_uniform(5, u) != L.caro_host_move_uniform(5, u, p) for u in range(50) for p in range(4))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_playthrough_share_is_binomial(p):
    L = _L()
    n = 100000
    k = sum(L.caro_host_resign_uniform(11, u) < p for u in range(n))
    sd = math.sqrt(n * p * (1 - p))
    assert abs(k - n * p) < 5 * sd, (k, n * p, sd)


def _game(q, z, playthrough=True):
    z = np.asarray(z)
    return {"q": np.asarray(q, np.float64), "z": z, "playthrough": playthrough, "resigned": bool(z[-1] == -1)}


# hand-built playthrough games (game order, z from each ply's mover's view) and one game that could resign
G1 = _game([0.5, -0.6, -0.9, 0.2], [1, -1, 1, -1])
G2 = _game([0.1, -0.8], [0, 0])                     # a draw
G3 = _game([0.3, 0.2, -0.4], [-1, 1, -1])
G4 = _game([-0.99], [1], playthrough=False)         # not a playthrough game: never counted
GAMES = [G1, G2, G3, G4]


def test_false_positive_rate_by_hand():
    from caro_ai_amd.resign import false_positive_rate
    # t = -0.5: G1 triggers at ply 1 (its mover lost: right), not at ply 2 (q = -0.9 too, but its mover won: only the
    # FIRST ply counts); G2 triggers at ply 1 and draws (a draw is a false positive); G3 never goes below -0.5
    assert false_positive_rate(GAMES, -0.5) == 0.5
    # t = -0.3: G1 ply 1 right, G2 ply 1 false, G3 ply 2 right
    assert false_positive_rate(GAMES, -0.3) == pytest.approx(1 / 3)
    # t = 0.55: every game triggers at ply 0: G1 (won) false, G2 (draw) false, G3 (lost) right
    assert false_positive_rate(GAMES, 0.55) == pytest.approx(2 / 3)
    # t = -0.95: no playthrough game triggers (G4 would, but it is not one): 0
    assert false_positive_rate(GAMES, -0.95) == 0.0
    assert false_positive_rate(GAMES, -1.0) == 0.0
    assert false_positive_rate([], 0.3) == 0.0


def test_calibrate_by_hand():
    from caro_ai_amd.resign import calibrate
    up = lambda x: float(np.nextafter(x, np.inf))  # noqa: E731
    # FP at the candidates (t = nextafter(q): q <= x triggers), worked out from G1..G3:
    #   -1: 0 | -0.9: 1 | -0.8: 1 | -0.6: 1/2 | -0.4: 1/3 | 0.1: 1/3 | 0.2: 2/3 | 0.3: 1/3 | 0.5: 2/3
    assert calibrate(GAMES, 0.34, current=0.0, min_games=3) == up(0.3)   # the LARGEST with FP <= target, not the first
    assert calibrate(GAMES, 0.2, current=0.0, min_games=3) == -1.0
    assert calibrate(GAMES, 0.5, current=0.0, min_games=3) == up(0.3)
    assert calibrate(GAMES, 0.7, current=0.0, min_games=3) == up(0.5)
    # fewer playthrough games than min_games: the current threshold stays (G4 does not count)
    assert calibrate(GAMES, 0.34, current=0.123, min_games=4) == 0.123
    assert calibrate([], 0.05, current=-0.8) == -0.8


def test_calibrate_sweep_matches_brute_force():
    """calibrate's interval sweep against false_positive_rate at every candidate, on random games"""
    from caro_ai_amd.resign import calibrate, false_positive_rate
    rng = np.random.default_rng(7)
    for trial in range(20):
        games = []
        for _ in range(int(rng.integers(20, 40))):
            n = int(rng.integers(1, 12))
            q = np.round(rng.uniform(-1, 1, n), 1)  # ties between games and inside a game
            z = rng.choice([-1, 0, 1], n)
            games.append(_game(q, z, playthrough=bool(rng.random() < 0.8)))
        pt = [g for g in games if g["playthrough"]]
        qs = np.concatenate([g["q"] for g in pt])
        cand = sorted(set([-1.0] + [float(np.nextafter(x, np.inf)) for x in qs if np.nextafter(x, np.inf) <= 1.0]))
        for target in (0.0, 0.2, 0.5):
            want = max(t for t in cand if false_positive_rate(games, t) <= target)
            assert calibrate(games, target, current=9.0, min_games=1) == want, (trial, target)


def test_split_games_by_hand():
    """a drain's rows: each game's plies last to first, games in record order; steps + 1 tuples per game"""
    from caro_ai_amd.resign import split_games
    drain = {
        "games": np.array([[7, 0, 1, 2], [9, 1, 1, 1]], np.int64),   # uid 7: 3 plies, won by player 0; uid 9: 2 plies
        "players": np.array([0, 1, 0, 1, 0], np.int32),
        "z": np.array([1, -1, 1, -1, 1], np.int32),                 # uid 9: player 1 resigned at its last ply
        "root_q": np.array([0.9, -0.2, 0.1, -0.7, 0.4]),
    }
    g7, g9 = split_games(drain)
    assert g7["uid"] == 7 and g7["steps"] == 2 and not g7["resigned"]
    assert g7["players"].tolist() == [0, 1, 0] and g7["z"].tolist() == [1, -1, 1] and g7["q"].tolist() == [0.1, -0.2, 0.9]
    assert g9["uid"] == 9 and g9["resigned"] and g9["playthrough"] is None
    assert g9["players"].tolist() == [0, 1] and g9["z"].tolist() == [1, -1] and g9["q"].tolist() == [0.4, -0.7]
    # with the engine's seed and playthrough share: the playthrough flag is the host export's
    L = _L()
    for g in split_games(drain, seed=3, playthrough=0.5):
        assert g["playthrough"] == (L.caro_host_resign_uniform(3, g["uid"]) < 0.5)
    bad = dict(drain, z=drain["z"][:4], players=drain["players"][:4], root_q=drain["root_q"][:4])
    with pytest.raises(ValueError):
        split_games(bad)


def test_summary_counts_every_game():
    from caro_ai_amd.resign import summary
    s = summary(GAMES, -0.5)
    assert s["resign_fraction"] == 2 / 4   # G1 and G3 end with their mover losing
    assert s["resign_false_positive"] == 0.5


def test_cli_resign_options_parse():
    from caro_ai_amd import train
    a = train.parse_args(["-n", "x", "-g", "0"])
    assert a.resign_threshold is None and a.resign_playthrough == 0.1 and a.resign_target_fp is None
    a = train.parse_args(["-n", "x", "-g", "0", "--resign-threshold", "-0.9", "--resign-playthrough", "0.2",
                          "--resign-target-fp", "0.05"])
    assert (a.resign_threshold, a.resign_playthrough, a.resign_target_fp) == (-0.9, 0.2, 0.05)
