"""Playout cap randomization on the CPU: the ply-class uniform of caro_noise.h (host export) against a plain-Python
statement and its binomial share, split_games carrying the ply classes, and the train CLI's two options."""
import math

import numpy as np
import pytest

from tests.synth_net import MASK, _mix64_py


def _L():
    from caro_ai_amd import _lib
    return _lib.load()


def _cap_uniform_py(seed, uid, ply):
    """caro_cap_uniform: mix64(mix64(mix64(seed ^ "pcap") + uid) ^ ply), 52 bits -> (0, 1)"""
    k = _mix64_py(seed ^ 0x70636170)
    k = _mix64_py((k + uid) & MASK)
    k = _mix64_py(k ^ ply)
    return ((k >> 12) + 0.5) * (1.0 / 4503599627370496.0)


def test_cap_uniform_is_its_python_statement():
    L = _L()
    rng = np.random.default_rng(5)
    seeds = [0, 1, 7, 2 ** 64 - 1, int(rng.integers(0, 2 ** 63))]
    uids = list(range(1000)) + [int(u) for u in rng.integers(0, 2 ** 63, 4000, dtype=np.int64)]
    plies = [0, 1, 2, 41, 224, 2 ** 32 - 1]
    for i, uid in enumerate(uids):
        seed, ply = seeds[i % len(seeds)], plies[(i // len(seeds)) % len(plies)]
        assert L.caro_host_cap_uniform(seed, uid, ply) == _cap_uniform_py(seed, uid, ply), (seed, uid, ply)
    # its own stream: neither the move uniform of the same ply nor the resignation uniform
    for u in range(50):
        for p in range(4):
            c = L.caro_host_cap_uniform(5, u, p)
            assert c != L.caro_host_move_uniform(5, u, p) and c != L.caro_host_resign_uniform(5, u)


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_full_share_is_binomial(p):
    L = _L()
    n = 100000
    k = sum(L.caro_host_cap_uniform(11, u // 50, u % 50) < p for u in range(n))  # 2 000 games x 50 plies
    sd = math.sqrt(n * p * (1 - p))
    assert abs(k - n * p) < 5 * sd, (k, n * p, sd)


def test_split_games_carries_full_in_game_order():
    from caro_ai_amd.resign import split_games
    drain = {
        "games": np.array([[7, 0, 1, 2], [9, 1, 0, 1]], np.int64),   # uid 7: 3 plies; uid 9: 2 plies
        "players": np.array([0, 1, 0, 1, 0], np.int32),
        "z": np.array([1, -1, 1, 0, 0], np.int32),
        "full": np.array([True, False, False, False, True]),         # rows: each game's plies last to first
    }
    g7, g9 = split_games(drain)
    assert g7["full"].tolist() == [False, False, True]
    assert g9["full"].tolist() == [True, False]
    assert "full" not in split_games({k: v for k, v in drain.items() if k != "full"})[0]


def test_cli_playout_cap_options_parse_and_default():
    from caro_ai_amd import config as cfg
    from caro_ai_amd import train
    a = train.parse_args(["-n", "x", "-g", "0"])
    assert a.playout_cap_full is None and a.playout_cap_fast is None
    assert train.playout_cap_from_args(a) is None
    a = train.parse_args(["-n", "x", "-g", "0", "--playout-cap-full", "0.25"])
    assert train.playout_cap_from_args(a) == (0.25, max(2, cfg.MCTS_SEARCHES // 5))
    assert train.playout_cap_from_args(a, searches=25) == (0.25, 5)
    a = train.parse_args(["-n", "x", "-g", "0", "--playout-cap-full", "0.5", "--playout-cap-fast", "3"])
    assert train.playout_cap_from_args(a) == (0.5, 3)
    for bad in (["--playout-cap-full", "1.5"], ["--playout-cap-full", "0.5", "--playout-cap-fast", "1"],
                ["--playout-cap-full", "0.5", "--playout-cap-fast", "11"], ["--playout-cap-fast", "3"]):
        with pytest.raises(SystemExit):
            train.playout_cap_from_args(train.parse_args(["-n", "x", "-g", "0"] + bad))
