"""Resignation on the GPU (include/caro_hip.h, "resignation"; SelfPlayEngine.set_resign): the recorded root Q is the
oracle's, a resigned game is the prefix of the game played without resignation, the threshold -1 changes nothing but
adds root_q, the sign of the rule, the argument checks, the real net, and the train CLI.

Thresholds are not hard-coded: each configuration is first played with recording on and resignation off (t = -1), and
t is taken from that run's per-game minimum root Q so that a share of the games that can resign does."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests.test_gpu_engine import DEV, _game_of, _oracle_of

pytestmark = pytest.mark.gpu

PLAYTHROUGH = 0.25


def _play(game, G, S, B, n_games, resign, seed=5, stagger=False, pool=False, one_call=False, uniforms=False,
          evict=False, evaluators=None, sbt0=10):
    """play exactly the games with local index < n_games (games_limit) and return {uid: game dict} (resign.split_games
    with states and pi), or, with resign None, the raw drains"""
    from caro_ai_amd import _lib
    from caro_ai_amd.engine import SelfPlayEngine
    from caro_ai_amd.net_hip import HashNet
    from caro_ai_amd.resign import split_games
    hw = game.obs_shape[1] * game.obs_shape[2]
    cap = None if evict else S * B * hw + 64
    eng = SelfPlayEngine(game, G, evaluators=evaluators or [HashNet(game, device=DEV)], max_batch=B,
                         steps_before_tau_0=sbt0, seed=seed, device=DEV, searches_hint=S, stagger=stagger,
                         stagger_recycle=(2 if pool else 1), games_limit=n_games, evict=evict, node_cap=cap)
    if resign is not None:
        eng.set_resign(*resign)
    L = _lib.load()
    drains, done = [], 0
    for _ in range((hw + 4) * (-(-n_games // G)) + S + 8):  # one pass = one ply per game (staggered: on average)
        if stagger:
            eng.search(S, B)
        elif one_call:
            eng.search_step(S, B)
        else:
            eng.search(S, B)
            u = None
            if uniforms:  # a table of our own, keyed by (uid, ply) so that both runs draw the same values per game
                _, _, plies, uid = eng.roots()
                u = [L.caro_host_move_uniform(seed + 1000, int(a), int(p)) for a, p in zip(uid, plies)]
            eng.step(uniforms=u)
        d = eng.drain(recycle=True)
        if d["games"].shape[0]:
            drains.append({k: v.cpu().numpy().copy() for k, v in d.items()})
            done += d["games"].shape[0]
        if done >= n_games:
            break
    c = eng.counters()
    eng.close()
    assert done == n_games and c["overflows"] == 0 and c["finished"] == n_games
    if resign is None:
        return drains, c
    games = {}
    for d in drains:
        for g in split_games(d, seed, resign[1]):
            assert g["uid"] not in games
            games[g["uid"]] = g
    return games, c


def _threshold(off):
    """t from the recording run: just above the median of the per-game minimum root Q of the games that can resign"""
    mins = sorted(float(g["q"].min()) for g in off.values() if not g["playthrough"])
    t = float(np.nextafter(mins[len(mins) // 2 - 1], np.inf))
    share = np.mean([m < t for m in mins])
    assert 0.2 <= share <= 0.8, (share, mins)
    return t


def _check_prefixes(off, on, t):
    """every game of the run with resignation against the same uid of the recording run"""
    assert sorted(off) == sorted(on)
    resigned = 0
    for uid, a in off.items():
        b = on[uid]
        hit = np.flatnonzero(a["q"] < t)
        if a["playthrough"] or not len(hit):
            for k in ("states", "players", "pi", "z", "q"):
                np.testing.assert_array_equal(a[k], b[k], err_msg="%s of uid %d" % (k, uid))
            assert (a["result"], a["steps"], a["first"]) == (b["result"], b["steps"], b["first"]), uid
            assert not b["resigned"] or a["resigned"]
            continue
        i = int(hit[0])
        resigned += 1
        assert b["resigned"] and b["steps"] == i and len(b["z"]) == i + 1, (uid, i, b["steps"])
        for k in ("states", "players", "pi", "q"):
            np.testing.assert_array_equal(a[k][:i + 1], b[k], err_msg="%s of uid %d" % (k, uid))
        np.testing.assert_array_equal(b["z"], [-1 if (i - j) % 2 == 0 else 1 for j in range(i + 1)])
        assert b["result"] == (-1 if b["players"][i] == 0 else 1) and b["first"] == a["first"]
    n_can = sum(not g["playthrough"] for g in off.values())
    assert 0.2 * n_can <= resigned <= 0.8 * n_can
    assert any(g["playthrough"] for g in off.values())
    return resigned


def _oracle_root_q(d, games, seed, S, B, n=8):
    """test 1: for n games, the oracle driven along the engine's states ply by ply; every tuple's root Q equals
    get_node(root)["Q"][first argmax N] bit for bit"""
    game = _game_of(d)
    for uid in sorted(games)[:n]:
        g = games[uid]
        o = _oracle_of(d)
        o.use_synth_net()
        o.set_stream(seed, uid)
        states = game.from_keys(np.ascontiguousarray(g["states"]).view(np.uint64))
        for i, (s, pl) in enumerate(zip(states, g["players"].tolist())):
            o.search_batch(S, B, s, pl, ply=i)
            node = o.get_node(s)
            best = int(np.argmax(node["N"]))
            assert g["q"][i] == node["Q"][best], (uid, i, g["q"][i], node["Q"][best])


C4 = {"kind": "c4"}


@pytest.mark.parametrize("form", ["stag_recycle", "stag_pool", "search_move", "step_uniforms"])
def test_connect4_resigned_games_are_prefixes(form):
    game = _game_of(C4)
    G, S, B, N, seed = 32, 4, 8, 64, 5
    kw = {"stag_recycle": dict(stagger=True), "stag_pool": dict(stagger=True, pool=True),
          "search_move": dict(one_call=True), "step_uniforms": dict(uniforms=True)}[form]
    off, _ = _play(game, G, S, B, N, (-1.0, PLAYTHROUGH), seed=seed, **kw)
    if form in ("stag_recycle", "search_move"):
        _oracle_root_q(C4, off, seed, S, B)
    t = _threshold(off)
    on, c = _play(game, G, S, B, N, (t, PLAYTHROUGH), seed=seed, **kw)
    _check_prefixes(off, on, t)
    assert c["plies"] == sum(len(g["z"]) for g in on.values())  # the resignation ply counts as a ply


def test_caro_7x7_staggered_resigned_games_are_prefixes():
    d = {"kind": "caro", "n": 7, "k": 4}
    game = _game_of(d)
    from caro_ai_amd.engine import staggered_geometry
    G, S, B, N, seed = 32, 3, 8, 48, 9
    assert staggered_geometry(game, B)
    off, _ = _play(game, G, S, B, N, (-1.0, PLAYTHROUGH), seed=seed, stagger=True)
    _oracle_root_q(d, off, seed, S, B)
    t = _threshold(off)
    on, _ = _play(game, G, S, B, N, (t, PLAYTHROUGH), seed=seed, stagger=True)
    _check_prefixes(off, on, t)


@pytest.mark.parametrize("stagger", [False, True])
def test_gomoku15_multiwave_with_eviction_resigned_games_are_prefixes(stagger):
    """15 x 15 k = 5 at 8 descents per minibatch: several wavefronts per game -- k_tree_mw (the ply in the closing
    launch, caro_search_move) and k_tree_stag_mw -- with eviction on"""
    d = {"kind": "mnk", "n": 15, "k": 5}
    game = _game_of(d)
    G, S, B, N, seed = 24, 2, 8, 24, 3
    kw = dict(stagger=True) if stagger else dict(one_call=True)
    off, _ = _play(game, G, S, B, N, (-1.0, PLAYTHROUGH), seed=seed, evict=True, **kw)
    if stagger:
        _oracle_root_q(d, off, seed, S, B, n=4)
    t = _threshold(off)
    on, _ = _play(game, G, S, B, N, (t, PLAYTHROUGH), seed=seed, evict=True, **kw)
    _check_prefixes(off, on, t)


@pytest.mark.parametrize("stagger", [False, True])
def test_threshold_minus_one_only_adds_root_q(stagger):
    """test 3: set_resign(-1, p) leaves every tuple byte-identical to an engine that never called it; only root_q is
    added to the drain"""
    game = _game_of(C4)
    kw = dict(stagger=True, pool=True) if stagger else dict(one_call=True)
    plain, c0 = _play(game, 32, 4, 8, 64, None, seed=7, **kw)
    from caro_ai_amd.engine import SelfPlayEngine
    from caro_ai_amd.net_hip import HashNet
    # the same run with recording on, as raw drains
    eng = SelfPlayEngine(game, 32, evaluators=[HashNet(game, device=DEV)], max_batch=8, steps_before_tau_0=10, seed=7,
                         device=DEV, searches_hint=4, stagger=stagger, stagger_recycle=2 if stagger else 1,
                         games_limit=64, node_cap=4 * 8 * 42 + 64)
    eng.set_resign(-1.0, 0.5)
    drains, done = [], 0
    while done < 64:
        if stagger:
            eng.search(4, 8)
        else:
            eng.search_step(4, 8)
        d = eng.drain(recycle=True)
        if d["games"].shape[0]:
            drains.append({k: v.cpu().numpy().copy() for k, v in d.items()})
            done += d["games"].shape[0]
    c1 = eng.counters()
    eng.close()
    assert c1 == c0
    assert len(drains) == len(plain)
    for a, b in zip(plain, drains):
        assert set(b) == set(a) | {"root_q"} and "root_q" not in a
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
        assert b["root_q"].shape == b["z"].shape and np.isfinite(b["root_q"]).all()
        assert (np.abs(b["root_q"]) <= 1).all()


def test_sign_double_threat_resigns_and_the_winner_does_not():
    """test 4: TicTacToe(3,3), player 1 holds two open lines (cells 2 and 6 win) and player 0 is to move: whatever it
    plays it loses, so at enough simulations its root Q is near -1 and it resigns at t = -0.5.  The same board with
    player 1 to move (it wins at once) does not resign."""
    from caro_ai_amd import _lib
    from caro_ai_amd.engine import SelfPlayEngine
    from caro_ai_amd.lib.game.tictactoe import TicTacToe
    from caro_ai_amd.net_hip import HashNet
    game = TicTacToe(3, 3)
    s = game.initial_state
    for cell, pl in [(0, 1), (5, 0), (1, 1), (7, 0), (3, 1)]:
        s, won = game.move(s, cell, pl)
        assert not won
    S, B = 100, 8
    eng = SelfPlayEngine(game, 2, evaluators=[HashNet(game, device=DEV)], max_batch=B, steps_before_tau_0=0, seed=1,
                         device=DEV, searches_hint=S, node_cap=S * B * 9 + 64)
    eng.set_resign(-0.5, 0.0)
    eng.set_roots([s, s], [0, 1])
    eng.search(S, B)
    actions, done, result = (x.cpu().numpy() for x in eng.step())
    assert actions[0] == _lib.RESIGNED and done[0] == 1 and result[0] == -1   # player 0 resigned: net1 result -1
    assert actions[1] in (2, 6) and done[1] == 1 and result[1] == -1          # player 1 won on the board
    keys, players, plies, _ = eng.roots()
    assert game.from_key(keys[0]) == s and players[0] == 0 and plies[0] == 1  # no move; the ply's tuple counts
    d = eng.drain(recycle=False)
    q, z = d["root_q"].cpu().numpy(), d["z"].cpu().numpy()
    assert len(z) == 2 and z.tolist() == [-1, 1]
    assert q[0] < -0.5 and q[1] > 0.5
    assert eng.counters()["overflows"] == 0
    eng.close()


def test_argument_checks():
    """test 5: NaN, t outside [-1, 1], playthrough outside [0, 1] -> CARO_E_INVAL; a _q drain before set_resign ->
    CARO_E_STATE"""
    from caro_ai_amd import _lib
    from caro_ai_amd.engine import SelfPlayEngine
    from caro_ai_amd.net_hip import HashNet
    L = _lib.load()
    game = _game_of(C4)
    for stagger in (False, True):
        eng = SelfPlayEngine(game, 8, evaluators=[HashNet(game, device=DEV)], max_batch=8, device=DEV, searches_hint=2,
                             stagger=stagger, node_cap=2 * 8 * 42 + 64)
        for t, p in [(math.nan, 0.1), (0.0, math.nan), (-1.0000001, 0.1), (1.5, 0.1), (0.0, -0.01), (0.0, 1.01),
                     (math.inf, 0.1)]:
            assert L.caro_engine_set_resign(eng.h, t, p) == -22, (t, p)
            with pytest.raises(ValueError):
                eng.set_resign(t, p)
        cap = 8 * 42
        bufs = [torch.zeros(n, dtype=dt, device=DEV) for n, dt in
                [(cap, torch.int64), (cap, torch.int32), (cap * 7, torch.float64), (cap, torch.int32),
                 (32, torch.int64), (cap, torch.float64)]]
        p = [C.c_void_p(b.data_ptr()) for b in bufs]
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if stagger:
            rc = L.caro_drain_parked_begin_q(eng.h, cap, p[0], p[1], p[2], p[3], p[4], p[5], st)
        else:
            rc = L.caro_drain_tuples_begin_q(eng.h, cap, p[0], p[1], p[2], p[3], p[4], 1, p[5], st)
        assert rc == -71
        assert eng.resign is None
        eng.set_resign(-1.0, 1.0)
        eng.set_resign(1.0, 0.0)
        assert eng.resign == (1.0, 0.0)
        eng.close()


def test_real_net_connect4_staggered_consistency():
    """test 6: the shipped best_026_12000.dat on the fused HIP net, staggered: a resigned game ends at the first ply
    of its own root_q below t, playthrough games never resign, a game that could resign and did not never went below
    t (consistency only: the bits depend on the net's launch shapes)"""
    import os
    from caro_ai_amd.lib.model import Net
    from caro_ai_amd.net_hip import HipNet
    from tests.conftest import GOLDEN
    game = _game_of(C4)
    net = Net(game.obs_shape, game.action_space)
    net.load_state_dict(torch.load(os.path.join(GOLDEN, "weights", "best_026_12000.dat"), map_location="cpu"))
    net = net.to(DEV).eval()
    G, S, B, N, seed = 64, 10, 8, 64, 21
    off, _ = _play(game, G, S, B, N, (-1.0, PLAYTHROUGH), seed=seed, stagger=True, evaluators=[HipNet(net, DEV)])
    mins = sorted(float(g["q"].min()) for g in off.values() if not g["playthrough"])
    t = float(np.nextafter(mins[len(mins) // 2], np.inf))
    on, _ = _play(game, G, S, B, N, (t, PLAYTHROUGH), seed=seed, stagger=True, evaluators=[HipNet(net, DEV)])
    n_res = 0
    for uid, g in on.items():
        hit = np.flatnonzero(g["q"] < t)
        if g["playthrough"]:
            assert not g["resigned"], uid
            continue
        if g["resigned"]:
            n_res += 1
            assert len(hit) and hit[0] == len(g["q"]) - 1, (uid, hit, len(g["q"]))
            assert g["result"] == (-1 if g["players"][-1] == 0 else 1)
        else:
            assert not len(hit), uid
    assert n_res > 0


def test_cli_resign_options_log_the_three_scalars(tmp_path, monkeypatch):
    """test 7: python -m caro_ai_amd.train with --resign-threshold / --resign-target-fp runs and logs resign_threshold,
    resign_fraction and resign_false_positive"""
    from caro_ai_amd import train
    rows = []

    class Writer:
        def add_scalar(self, name, value, step):
            rows.append((name, float(value), step))

        def close(self):
            pass

    monkeypatch.setattr(train, "_writer", lambda name: Writer())
    train.main(["-n", "r", "-g", "0", "--cuda", "--games", "64", "--iterations", "1", "--saves", str(tmp_path),
                "--resign-threshold", "-0.9", "--resign-playthrough", "0.2", "--resign-target-fp", "0.05"])
    names = {r[0] for r in rows}
    assert {"resign_threshold", "resign_fraction", "resign_false_positive"} <= names
    got = {r[0]: r[1] for r in rows}
    assert got["resign_threshold"] == -0.9
    assert 0.0 <= got["resign_fraction"] <= 1.0 and 0.0 <= got["resign_false_positive"] <= 1.0
