"""Paired random openings for arena matches on the GPU (include/caro_hip.h, "openings", caro_engine_set_opening_pairs;
SelfPlayEngine.set_openings(..., paired=True)): the roots of an engine with two nets and two stores at every game start
against the rule in plain Python; whole arena games in every schedule against the game composed on the oracle from its
opened root (tests/arena_openings_ref.py); unpaired openings in an arena engine; the flag is neutral where it has to be;
the refusals; the product path (play_games, train.evaluate) and the two CLIs.

Every engine here evaluates with two table nets (HashNet, salts 0x1111 / 0x2222), the oracle with their twins
(use_synth_net), unless said otherwise.  Games are those of seed 5, uids 7100 .., first player = uid & 1; every
comparison is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from caro_ai_amd import openings
from tests.arena_openings_ref import compose_arena_game
from tests.test_gpu_engine import DEV, _game_of, _oracle_of

pytestmark = pytest.mark.gpu

C4 = {"kind": "c4"}
MNK5 = {"kind": "mnk", "n": 5, "k": 4}
CARO7 = {"kind": "caro", "n": 7, "k": 4}
SEED, BASE, SALTS, MP = 5, 7100, (0x1111, 0x2222), 6
E_INVAL, E_STATE = -22, -71


def _arena(game, G, S=5, B=8, stagger=False, pool=False, n_games=0, first_player_mode=2, evaluators=None, seed=SEED):
    """an arena engine: two nets, two stores, tau = 0 from move 0"""
    from caro_ai_amd.engine import SelfPlayEngine
    from caro_ai_amd.net_hip import HashNet
    hw = game.obs_shape[1] * game.obs_shape[2]
    evs = evaluators or [HashNet(game, device=DEV, salt=s) for s in SALTS]
    return SelfPlayEngine(game, G, evaluators=evs, n_stores=2, max_batch=B, steps_before_tau_0=0, seed=seed,
                          uid_base=BASE, first_player_mode=first_player_mode, device=DEV, searches_hint=S,
                          stagger=stagger, stagger_recycle=(2 if pool else 1), games_limit=n_games,
                          node_cap=S * B * hw + 64)


def _roots(eng):
    keys, players, ply, uid = eng.roots()
    return list(eng.game.from_keys(keys)), players.tolist(), ply.tolist(), uid.tolist()


def _rule(game, uids, mp, paired, seed=SEED):
    return [openings.opening(game, seed, u, u & 1, mp, paired=paired) for u in uids]


def _assert_twins(game, want):
    """consecutive games (even uid first): the same count, opposite movers, the same planes each for its own mover"""
    for (s0, p0, m0), (s1, p1, m1) in zip(want[0::2], want[1::2]):
        planes = game.states_to_training_batch([s0, s1], [p0, p1])
        assert m0 == m1 and p0 == 1 - p1 and np.array_equal(planes[0], planes[1])


def _play(eng, S, B, n_games, stagger=False, one_call=False, before_pass=None):
    """play exactly n_games games; returns ({uid: game dict}, raw drains, counters)"""
    from caro_ai_amd.resign import split_games
    hw = eng.HW
    drains, done = [], 0
    for n in range((hw + 4) * (-(-n_games // eng.G)) + S + 8):
        if before_pass is not None:
            before_pass(n, eng)
        if stagger:
            eng.search(S, B)
        elif one_call:
            eng.search_step(S, B)
        else:
            eng.search(S, B)
            eng.step()
        d = eng.drain(recycle=True)
        if d["games"].shape[0]:
            drains.append({k: v.cpu().numpy().copy() for k, v in d.items()})
            done += d["games"].shape[0]
        if done >= n_games:
            break
    c = eng.counters()
    assert done == n_games and c["overflows"] == 0 and c["finished"] == n_games
    games = {}
    for d in drains:
        for g in split_games(d):
            assert g["uid"] not in games
            games[g["uid"]] = g
    return games, drains, c


def _tuple0(game, g):
    return (game.from_keys(np.ascontiguousarray(g["states"][:1]).view(np.uint64))[0], int(g["players"][0]),
            int(g["open"][0]))


FORMS = {"search_step": dict(), "search_move": dict(one_call=True), "staggered": dict(stagger=True),
         "staggered_pool": dict(stagger=True, pool=True)}
ROOT_CASES = [(C4, "search_move"), (C4, "staggered"), (C4, "staggered_pool"), (MNK5, "search_step"), (MNK5, "staggered"),
              (CARO7, "search_move"), (CARO7, "staggered")]


@pytest.mark.parametrize("d,form", ROOT_CASES, ids=["%s-%s" % (d["kind"], f) for d, f in ROOT_CASES])
def test_roots_follow_the_paired_rule_at_every_game_start(d, form):
    """test 1: after set_openings(6, paired=True) the roots equal the Python rule per uid and consecutive uids are twins;
    again after restart(); and at the starts inside a run -- the drain's recycle (lock-step), park_and_restart
    (staggered), k_stag_assign (staggered pool) -- 8 slots playing 16 games"""
    game = _game_of(d)
    kw = dict(FORMS[form])
    pool = kw.pop("pool", False)
    stagger = kw.get("stagger", False)
    if d is CARO7 and stagger:
        from caro_ai_amd.engine import staggered_geometry
        assert staggered_geometry(game, 8) and 8 * 64 > 64  # 8 descents x 64 lanes: k_tree_stag_mw
    G = 16
    eng = _arena(game, G, stagger=stagger, pool=pool)
    assert eng.opening_pairs is False
    s, p, _, u = _roots(eng)
    assert u == list(range(BASE, BASE + G)) and set(s) == {game.initial_state} and p == [x & 1 for x in u]
    eng.set_openings(MP, paired=True)
    assert eng.opening_pairs is True and eng.openings == MP
    want = _rule(game, u, MP, True)
    s, p, ply, _ = _roots(eng)
    assert list(zip(s, p)) == [w[:2] for w in want] and ply == [0] * G
    _assert_twins(game, want)
    assert any(w[2] & 1 for w in want) and any(w[2] == 0 for w in want) and max(w[2] for w in want) >= 3
    assert want != _rule(game, u, MP, False)
    # the two calls in the other order, from the plain key: pairs off re-opens under uid, on again under uid >> 1
    eng.set_openings(MP, paired=False)
    s, p, _, _ = _roots(eng)
    assert list(zip(s, p)) == [w[:2] for w in _rule(game, u, MP, False)]
    assert eng.L.caro_engine_set_opening_pairs(eng.h, 1) == 0
    eng.opening_pairs = True
    s, p, _, _ = _roots(eng)
    assert list(zip(s, p)) == [w[:2] for w in want]
    # restart keeps both settings
    eng.search(5, 8)
    if not stagger:
        eng.step()
    eng.restart(seed=SEED + 1)
    assert eng.opening_pairs is True
    s, p, ply, u2 = _roots(eng)
    want = _rule(game, u2, MP, True, seed=SEED + 1)
    assert u2 == u and list(zip(s, p)) == [w[:2] for w in want] and ply == [0] * G
    _assert_twins(game, want)
    eng.close()
    # the starts inside a run
    eng = _arena(game, 8, stagger=stagger, pool=pool, n_games=16)
    eng.set_openings(MP, paired=True)
    games, _, _ = _play(eng, 5, 8, 16, **kw)
    eng.close()
    uids = sorted(games)
    assert uids == list(range(BASE, BASE + 16))
    want = _rule(game, uids, MP, True)
    for uid, w in zip(uids, want):
        assert _tuple0(game, games[uid]) == w and games[uid]["first"] == w[1], uid
    _assert_twins(game, want)
    assert any(w[2] & 1 for w in want[8:]) and max(w[2] for w in want[8:]) >= 2


_COMPOSED = {}


def _composed(uid, paired, mp=MP, S=5, B=8):
    key = (uid, paired, mp, S, B)
    if key not in _COMPOSED:
        _COMPOSED[key] = compose_arena_game(lambda: _oracle_of(C4, 2), _game_of(C4), SEED, uid, uid & 1, mp, S, B, 0,
                                            SALTS, paired=paired)
    return _COMPOSED[key]


def _assert_game(game, g, want, uid):
    states = game.from_keys(np.ascontiguousarray(g["states"]).view(np.uint64))
    assert list(states) == want["states"], uid
    np.testing.assert_array_equal(g["players"], want["players"], err_msg="players of uid %d" % uid)
    assert g["pi"].dtype == np.float64 and g["open"].dtype == np.int16
    np.testing.assert_array_equal(g["pi"], want["pi"], err_msg="pi of uid %d" % uid)
    np.testing.assert_array_equal(g["z"], want["z"], err_msg="z of uid %d" % uid)
    assert (g["open"] == want["open"]).all() and len(g["open"]) == len(want["z"]), uid
    assert (g["result"], g["steps"], g["first"]) == (want["result"], want["steps"], want["first"]), uid


def _check_composition(games, counters, paired):
    game = _game_of(C4)
    uids = sorted(games)
    want = [_composed(uid, paired) for uid in uids]
    for uid, w in zip(uids, want):
        _assert_game(game, games[uid], w, uid)
    assert counters["sims"] == sum(w["counters"]["sims"] for w in want)
    assert counters["expansions"] == sum(w["counters"]["expansions"] for w in want)
    return want


@pytest.mark.parametrize("form,G,N", [("search_step", 8, 16), ("search_move", 8, 16), ("staggered", 8, 8)])
def test_connect4_arena_games_match_the_oracle_composition(form, G, N):
    """test 2: S = 5, B = 8, tau = 0 from move 0; 16 games on 8 slots in the lock-step forms, 8 on 8 staggered"""
    game = _game_of(C4)
    kw = FORMS[form]
    eng = _arena(game, G, stagger=kw.get("stagger", False), n_games=N)
    eng.set_openings(MP, paired=True)
    games, _, c = _play(eng, 5, 8, N, **kw)
    eng.close()
    assert sorted(games) == list(range(BASE, BASE + N))
    want = _check_composition(games, c, True)
    # an odd count: the mover of tuple 0 is not uid & 1 there
    odd = [(uid, w) for uid, w in zip(sorted(games), want) if w["open"] & 1]
    assert odd and all(w["first"] != (uid & 1) for uid, w in odd)
    # the two games of a pair: one opening, played from both sides
    for a, b in zip(want[0::2], want[1::2]):
        assert a["open"] == b["open"] and a["first"] == 1 - b["first"]
    assert any(not np.array_equal(a["pi"], b["pi"]) for a, b in zip(want[0::2], want[1::2]))  # independent noise


def test_unpaired_openings_in_an_arena_engine_are_keyed_by_uid():
    """test 3: the roots and the games are those of key uid"""
    game = _game_of(C4)
    eng = _arena(game, 8, n_games=16)
    eng.set_openings(MP)
    assert eng.opening_pairs is False
    s, p, _, u = _roots(eng)
    assert list(zip(s, p)) == [w[:2] for w in _rule(game, u, MP, False)]
    games, _, c = _play(eng, 5, 8, 16, one_call=True)
    eng.close()
    want = _check_composition(games, c, False)
    assert [w["open"] for w in want] != [_composed(uid, True)["open"] for uid in sorted(games)]


def _same_bytes(a, b, keys):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("form", ["search_move", "staggered"])
def test_the_flag_is_neutral_without_openings(form):
    """test 4a: pairs on with max_plies 0, and pairs on then off again before any launch, each drain the tuples of an
    engine that never made the call, bit for bit"""
    game = _game_of(C4)
    kw = FORMS[form]

    def run(prepare):
        eng = _arena(game, 8, stagger=kw.get("stagger", False), n_games=16)
        prepare(eng)
        _, drains, c = _play(eng, 5, 8, 16, **kw)
        eng.close()
        return drains, c

    def on_then_off(eng):
        eng.set_openings(MP, paired=True)
        assert _roots(eng)[0] != [game.initial_state] * 8
        eng.set_openings(0, paired=False)
        assert eng.opening_pairs is False

    never, c0 = run(lambda eng: None)
    zero, c1 = run(lambda eng: eng.set_openings(0, paired=True))
    back, c2 = run(on_then_off)
    assert c0 == c1 == c2 and len(never) == len(zero) == len(back)
    for a, b, c in zip(never, zero, back):
        assert set(a) == set(b) and "open" not in a
        _same_bytes(a, b, a)
        assert set(c) == set(a) | {"open"} and not c["open"].any()
        _same_bytes(a, c, a)


def test_a_set_call_in_mid_run_leaves_games_in_flight_alone():
    """test 4b: after three passes every first game is in flight and keeps its root, the empty board; the games that
    start later are opened in pairs"""
    game = _game_of(C4)
    G, N = 8, 24

    def hook(n, eng):
        if n == 3:
            eng.set_openings(MP, paired=True)

    eng = _arena(game, G, n_games=N)
    games, _, _ = _play(eng, 5, 8, N, one_call=True, before_pass=hook)
    eng.close()
    later = 0
    for uid, g in games.items():
        if uid < BASE + G:
            assert _tuple0(game, g) == (game.initial_state, uid & 1, 0), uid
        else:
            assert _tuple0(game, g) == openings.opening(game, SEED, uid, uid & 1, MP, paired=True), uid
            later += int(g["open"][0] > 0)
    assert later >= 6


def test_refusals_change_no_root():
    """test 5: first_player_mode other than 2, a pending select, on outside {0, 1}"""
    from caro_ai_amd import _lib
    from tests.synth_net import SynthNet
    game = _game_of(C4)
    L = _lib.load()
    # first_player_mode 0: the library refuses, the Python layer before it
    eng = _arena(game, 8, first_player_mode=0)
    eng.set_openings(MP)
    before = _roots(eng)
    assert L.caro_engine_set_opening_pairs(eng.h, 1) == E_STATE
    assert b"first_player_mode" in L.caro_last_error()
    assert L.caro_engine_set_opening_pairs(eng.h, 0) == E_STATE
    with pytest.raises(ValueError, match="first_player_mode"):
        eng.set_openings(MP, paired=True)
    assert eng.opening_pairs is False and _roots(eng) == before
    eng.close()
    assert L.caro_engine_set_opening_pairs(None, 1) == E_INVAL
    # on = 2; a pending caro_select (the step-wise form: host-evaluated nets)
    evs = [SynthNet(84, 7, DEV, s) for s in SALTS]
    eng = _arena(game, 8, evaluators=evs)
    eng.set_openings(MP)
    before = _roots(eng)
    assert before[0] != [game.initial_state] * 8
    for bad in (2, -1):
        assert L.caro_engine_set_opening_pairs(eng.h, bad) == E_INVAL
    assert _roots(eng) == before
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.caro_select(eng.h, 8, 0, None, C.c_void_p(eng.planes.data_ptr()), C.c_void_p(eng.leaf_keys.data_ptr()),
                         st) == 0
    assert L.caro_engine_set_opening_pairs(eng.h, 1) == E_STATE
    with pytest.raises(_lib.CaroError):
        eng.set_openings(MP, paired=True)
    assert eng.opening_pairs is False
    assert L.caro_select_cancel(eng.h) == 0
    assert _roots(eng) == before
    # restart to another first_player_mode while the pairs are on
    eng.restart()
    eng.set_openings(MP, paired=True)
    with pytest.raises(_lib.CaroError, match="paired openings"):
        eng.restart(first_player_mode=0)
    eng.close()


def _weights(name):
    from tests.conftest import GOLDEN
    return os.path.join(GOLDEN, "weights", name)


def test_product_path_evaluate_and_play_games():
    """test 6: train.evaluate with opening_plies on the shipped Connect4 checkpoints; play_games' results do not depend
    on the number of slots"""
    from caro_ai_amd import match_stats, play, train
    from caro_ai_amd.lib import utils
    game = _game_of(C4)
    a = play.load_checkpoint(game, _weights("best_025_10600.dat"), DEV)
    b = play.load_checkpoint(game, _weights("best_026_12000.dat"), DEV)
    ratio, (w, l, d), s = train.evaluate(game, a, b, rounds=8, device=DEV, seed=3, opening_plies=4, counts=True,
                                         stats=True)
    assert w + l + d == 8 and ratio == w / 8
    assert (s["games"], s["pairs"], s["wins"], s["losses"], s["draws"], s["ratio"]) == (8, 4, w, l, d, ratio)
    assert train.evaluate(game, a, b, rounds=8, device=DEV, seed=3, opening_plies=4) == ratio
    r2, s2 = train.evaluate(game, a, b, rounds=8, device=DEV, seed=3, opening_plies=4, stats=True)
    assert r2 == ratio and s2 == s
    kw = dict(steps_before_tau_0=0, mcts_searches=20, mcts_batch_size=16, seed=3, uid_base=0, device=DEV, openings=4,
              opening_pairs=True)
    res8, st8 = utils.play_games(game, 8, None, a, b, concurrent=8, return_stats=True, **kw)
    res4 = utils.play_games(game, 8, None, a, b, concurrent=4, **kw)
    assert res8 == res4 and len(res8) == 8
    table = match_stats.pair_table(res8)
    assert int(table.sum()) == 4 and match_stats.summary(table) == s
    assert 0.0 < st8["open_plies_mean"] <= 4.0 and st8["open_games"] % 2 == 0
    # without the flag evaluate is what it was: the same number, and stats=True only appends
    plain = train.evaluate(game, a, b, rounds=8, device=DEV, seed=3)
    r3, s3 = train.evaluate(game, a, b, rounds=8, device=DEV, seed=3, stats=True)
    assert r3 == plain and s3["games"] == 8 and "pairs" not in s3 and s3["ratio"] == plain


TALLY = r"^%s vs %s -> w=\d+, l=\d+, d=\d+$"


def test_play_cli_prints_the_match_line_after_the_tally(capsys):
    """test 7a: with --opening-plies one match line follows every tally line; without it the output is today's"""
    from caro_ai_amd import play
    a, b = _weights("best_025_10600.dat"), _weights("best_026_12000.dat")
    play.main(["-g", "0", "--cuda", a, b, "-r", "4", "--opening-plies", "4"])
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 7 and out[4] == "Leaderboard:"
    for i, (x, y) in ((0, (a, b)), (2, (b, a))):
        assert re.match(TALLY % (re.escape(x), re.escape(y)), out[i]), out[i]
        m = re.match(r"^match: score=(\d\.\d{4}), pairs=2, split=(\d), se_pairs=\d\.\d{4} \(se_games=\d\.\d{4}\), "
                     r"elo=\S+ \[\S+, \S+\]$", out[i + 1])
        assert m, out[i + 1]
        w, l, d = (int(v) for v in re.findall(r"=(\d+)", out[i].split("->")[1]))
        assert w + l + d == 4 and float(m.group(1)) == round((w + d / 2) / 4, 4)
    play.main(["-g", "0", "--cuda", a, b, "-r", "4"])
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 5 and out[2] == "Leaderboard:" and not any("match" in line for line in out)
    assert re.match(TALLY % (re.escape(a), re.escape(b)), out[0]) and re.match(TALLY % (re.escape(b), re.escape(a)), out[1])
    for line in out[3:]:
        assert re.match(r"^\S+: \t w=\d+, l=\d+, d=\d+$", line), line


def test_train_cli_eval_opening_plies_runs_and_is_logged(tmp_path, monkeypatch):
    """test 7b: python -m caro_ai_amd.train --eval-opening-plies 4 for one tiny iteration whose gate runs"""
    from caro_ai_amd import train
    rows, lines = [], []

    class Writer:
        def add_scalar(self, name, value, step):
            rows.append((name, float(value), step))

        def close(self):
            pass

    monkeypatch.setattr(train, "_writer", lambda name: Writer())
    monkeypatch.setattr("builtins.print", lambda *a, **k: lines.append(" ".join(str(x) for x in a)))
    for name, value in (("EVALUATE_EVERY_STEP", 1), ("EVALUATION_ROUNDS", 4), ("MIN_REPLAY_TO_TRAIN", 256),
                        ("TRAIN_ROUNDS", 1)):
        monkeypatch.setattr(train.cfg, name, value)
    train.main(["-n", "r", "-g", "0", "--cuda", "--games", "64", "--iterations", "1", "--saves", str(tmp_path),
                "--eval-opening-plies", "4"])
    got = {r[0]: r[1] for r in rows}
    assert {"eval_win_ratio", "eval_score", "eval_se_pairs", "eval_elo", "eval_split_pairs"} <= set(got)
    assert 0.0 <= got["eval_win_ratio"] <= got["eval_score"] <= 1.0 and got["eval_win_ratio"] * 4 == round(got["eval_win_ratio"] * 4)
    assert 0 <= got["eval_split_pairs"] <= 2 and got["eval_se_pairs"] >= 0.0
    assert any(line.startswith("Net evaluated from paired openings, match: score=") for line in lines)
    assert any(line.startswith("Net evaluated, win ratio = ") for line in lines)
