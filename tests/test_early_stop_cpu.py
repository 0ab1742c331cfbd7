"""Early stop of decided tau = 0 plies, the parts that need no GPU (include/caro_hip.h, "early stop"): the decided
predicate on constructed rows, the oracle composition helper against a hand-worked case, and the host-side plumbing."""
import ctypes as C

import numpy as np
import pytest

from caro_ai_amd import early_stop
from tests.early_stop_ref import compose_game, tally


def test_decided_predicate_on_constructed_rows():
    M, B = 6, 8
    # m = 1: (M - m) * B = 40 simulations left; strict
    assert not early_stop.decided([50, 10, 0, 0, 0, 0, 0], 1, M, B)   # lead 40
    assert early_stop.decided([51, 10, 0, 0, 0, 0, 0], 1, M, B)       # lead 41
    # a tie for the first maximum: n2 = n1, never decided
    assert not early_stop.decided([90, 90, 0], 4, M, B)
    # the runner-up may sit before or after the best
    assert early_stop.decided([10, 0, 27], 4, M, B) and not early_stop.decided([10, 0, 26], 4, M, B)
    assert early_stop.decided([0, 27, 10], 4, M, B)
    # a single action: n2 = 0
    assert early_stop.decided([17], 4, M, B) and not early_stop.decided([16], 4, M, B)
    # an all-zero root, an absent root
    assert not early_stop.decided([0] * 7, 4, M, B)
    assert not early_stop.decided(None, 4, M, B) and not early_stop.decided([], 4, M, B)
    # m at both ends of its range: min_minibatches <= m <= M - 2
    big = [1000, 0, 0]
    assert early_stop.decided(big, 1, M, B, 1) and not early_stop.decided(big, 0, M, B, 1)
    assert early_stop.decided(big, 4, M, B, 1) and not early_stop.decided(big, 5, M, B, 1)
    assert early_stop.decided(big, 3, M, B, 3) and not early_stop.decided(big, 2, M, B, 3)
    assert not early_stop.decided(big, 4, M, B, 5)   # a floor above M - 2 never fires
    assert not early_stop.decided(big, 0, 2, B, 1)   # M = 2: no m in [1, 0]


def test_floor_validation():
    assert early_stop.floor(1) == 1 and early_stop.floor(np.int64(7)) == 7
    for bad in (0, -1, 1.5, 2.0, True, None, "3"):
        with pytest.raises(ValueError):
            early_stop.floor(bad)


def _tictactoe():
    from oracle.oracle import Oracle
    return Oracle(Oracle.MNK, 3, 3)


def test_composition_against_a_hand_worked_case():
    """3 x 3, S = 6, B = 4, tau = 0 from ply 0: the composed game is checked against its own definition, step by
    step, with plain oracle calls: at every ply the recorded count is the first decided m + 1 (or S), the N rows that
    decide are those of a replayed tree, and the move is the argmax of the FULL budget's N on the same tree -- the
    guarantee of the rule"""
    from oracle.oracle import move_uniform, sample_index
    seed, uid, S, B = 7, 3, 6, 4
    g = compose_game(_tictactoe, seed, uid, 1, S, B, 0)
    n = len(g["mb"])
    assert n >= 5 and all(g["tau0"]) and g["budget"] == [S] * n
    assert any(m < S for m in g["mb"]) and any(m == S for m in g["mb"])   # (3 x 3: wins in reach decide plies)

    def replay(i, extra):
        o = _tictactoe()
        o.use_synth_net()
        o.set_stream(seed, uid)
        for j in range(i):
            o.search_batch(g["mb"][j], B, g["states"][j], g["players"][j], ply=j)
        if extra:
            o.search_batch(extra, B, g["states"][i], g["players"][i], ply=i)
        node = o.get_node(g["states"][i])
        return o, (node["N"] if node is not None else np.zeros(9, np.int32))

    for i in range(n):
        first = None
        for m in range(1, S - 1):
            N = replay(i, m)[1]
            srt = np.sort(N)[::-1]
            lead = int(srt[0]) - int(srt[1])
            if lead > (S - m) * B and (N == srt[0]).sum() == 1:   # the rule, written out
                first = m
                break
        assert g["mb"][i] == (first + 1 if first is not None else S), i
        o, N_cut = replay(i, g["mb"][i])
        _, N_full = replay(i, S)
        assert int(np.argmax(N_cut)) == int(np.argmax(N_full)), i     # the guarantee
        pi = o.get_policy(g["states"][i], 0)
        np.testing.assert_array_equal(pi, g["pi"][i])
        assert pi[int(np.argmax(N_full))] == 1.0 and pi.sum() == 1.0
        if i + 1 < n:
            s2, won = o.move(g["states"][i], sample_index(pi, move_uniform(seed, uid, i)), g["players"][i])
            assert s2 == g["states"][i + 1] and not won
    t = tally([g])
    assert t["cut"] == sum(m < S for m in g["mb"]) and t["saved"] == sum(S - m for m in g["mb"])
    # early=False is the plain reference game
    o = _tictactoe()
    o.use_synth_net()
    o.set_stream(seed, uid)
    ref = o.play_game(0, S, B, 1)
    plain = compose_game(_tictactoe, seed, uid, 1, S, B, 0, early=False)
    assert plain["states"] == ref["states"] and plain["mb"] == [S] * ref["plies"]
    np.testing.assert_array_equal(plain["pi"], ref["pi"])


def test_tau1_plies_are_never_cut():
    g = compose_game(_tictactoe, 7, 3, 1, 6, 4, 100)
    assert g["mb"] == [6] * len(g["mb"]) and not any(g["tau0"])


def test_split_games_and_stop_stats_carry_mb():
    from caro_ai_amd.resign import split_games
    # two games: steps 2 (3 tuples) and 0 (1 tuple); rows last ply first
    d = {"games": np.array([[5, 0, 1, 2], [6, 1, -1, 0]], np.int64), "z": np.array([1, -1, 1, 1], np.int32),
         "players": np.array([0, 1, 0, 1], np.int32), "mb": np.array([3, 6, 6, 2], np.int16),
         "full": np.array([True, True, False, True])}
    g = split_games(d)
    assert g[0]["mb"].tolist() == [6, 6, 3] and g[1]["mb"].tolist() == [2]
    np.testing.assert_array_equal(early_stop.ply_indices(d["games"]), [2, 1, 0, 0])
    # sbt0 = 1: tau = 0 plies are the ply indices >= 1; S = 6: cut plies are rows 0 and 3
    st = early_stop.stop_stats([{k: d[k] for k in ("games", "mb")}], 6, 1)
    assert st == {"stop_plies": 2, "stop_tau0_plies": 2, "stop_minibatches_saved": 3 + 4}
    # with the cap's classes a fast ply (row 2) has the budget min(fast, searches); sbt0 = 0: every ply is tau = 0
    st = early_stop.stop_stats([d], 6, 0, fast=6)
    assert st == {"stop_plies": 2, "stop_tau0_plies": 4, "stop_minibatches_saved": 7}


def test_abi_declares_the_entry_points():
    from caro_ai_amd import _lib
    for name in ("caro_engine_set_early_stop", "caro_drain_tuples_begin_ex", "caro_drain_parked_begin_ex"):
        assert name in _lib.EXPORTS
    L = _lib.load()
    assert L.caro_engine_set_early_stop(None, 1) == -22   # null engine: CARO_E_INVAL, no GPU needed
    ex = _lib.CaroDrainExtra()
    assert ex.size == C.sizeof(_lib.CaroDrainExtra) and not ex.minibatches_dev
    # the struct of include/caro_hip.h: u32 size, then three pointers
    assert _lib.CaroDrainExtra.root_q_dev.offset == 8 and C.sizeof(_lib.CaroDrainExtra) == 32


def test_cli_option():
    from caro_ai_amd import train
    base = ["-n", "x", "-g", "0"]
    assert train.parse_args(base).early_stop is None
    assert train.parse_args(base + ["--early-stop"]).early_stop == 1
    assert train.parse_args(base + ["--early-stop", "4"]).early_stop == 4
