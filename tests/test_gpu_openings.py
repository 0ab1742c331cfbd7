"""Random openings on the GPU (include/caro_hip.h, "openings"; SelfPlayEngine.set_openings): the device function on every
lane geometry against the host helper; whole games in every schedule against the game composed on the oracle from its
opened root (tests/openings_ref.py); off and never-called are today's engine; what a set call (re)opens; the other
extensions on top of it; the staggered run at 1 024 slots; the training path and the train CLI.

Every engine here evaluates with the table net (HashNet), the oracle with its twin (use_synth_net), unless said
otherwise.  Games are those of seed 5, uids 0 .. n-1, first player = uid & 1."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.openings_ref import compose_game_from, host_opening, kind_of
from tests.test_gpu_engine import DEV, _game_of, _oracle_of
from tests.test_gpu_resign import _check_prefixes

pytestmark = pytest.mark.gpu

C4 = {"kind": "c4"}
SEED = 5


def _host_keys(game, seed, uids, firsts, max_plies):
    """caro_host_opening over arrays -> (keys u64[M, KW], players, made)"""
    from caro_ai_amd import _lib
    L = _lib.load()
    kind, n, k = kind_of(game)
    KW = game.key_words
    keys = np.zeros((len(uids), KW), np.uint64)
    players, made = np.zeros(len(uids), np.int32), np.zeros(len(uids), np.int32)
    key = (C.c_uint64 * 8)()
    p, m = C.c_int(), C.c_int()
    for i, (uid, fp) in enumerate(zip(uids.tolist(), firsts.tolist())):
        assert L.caro_host_opening(kind, n, k, seed, uid, fp, max_plies, key, C.byref(p), C.byref(m)) == 0
        keys[i], players[i], made[i] = key[:KW], p.value, m.value
    return keys, players, made


GEOMETRIES = ([{"kind": "mnk", "n": n, "k": min(n, 5)} for n in (3, 4, 5, 7, 9, 12, 15)] +
              [{"kind": "caro", "n": 4, "k": k} for k in (2, 3, 4)] +
              [{"kind": "caro", "n": 7, "k": 4}, {"kind": "caro", "n": 15, "k": 5}, C4])


@pytest.mark.parametrize("d", GEOMETRIES, ids=lambda d: "-".join(str(v) for v in d.values()))
def test_device_openings_equal_the_host_helper(d):
    """test 1: caro_openings_batch, one game per thread, 4 096 uids (64 blocks; the last uids beyond 2^32), a small cap
    and the largest one (connect four: also the largest its board allows)"""
    from caro_ai_amd import _lib
    L = _lib.load()
    game = _game_of(d)
    kind, n, k = kind_of(game)
    M, KW = 4096, game.key_words
    uids = np.arange(M, dtype=np.uint64)
    uids[-64:] += np.uint64(1 << 40)
    firsts = (np.arange(M) % 3 == 0).astype(np.int32)
    caps = {3, min(64, game.action_space - 1)} | ({41} if d is C4 else set())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    u_dev = torch.from_numpy(uids.view(np.int64)).to(DEV)
    f_dev = torch.from_numpy(firsts).to(DEV)
    for mp in sorted(caps):
        keys = torch.full((M, KW), -1, dtype=torch.int64, device=DEV)
        players = torch.full((M,), -1, dtype=torch.int32, device=DEV)
        made = torch.full((M,), -1, dtype=torch.int32, device=DEV)
        _lib.check(L.caro_openings_batch(kind, n, k, SEED, mp, M, C.c_void_p(u_dev.data_ptr()),
                                         C.c_void_p(f_dev.data_ptr()), C.c_void_p(keys.data_ptr()),
                                         C.c_void_p(players.data_ptr()), C.c_void_p(made.data_ptr()), st))
        wk, wp, wm = _host_keys(game, SEED, uids, firsts, mp)
        np.testing.assert_array_equal(made.cpu().numpy(), wm, err_msg="made at cap %d" % mp)
        np.testing.assert_array_equal(players.cpu().numpy(), wp, err_msg="players at cap %d" % mp)
        np.testing.assert_array_equal(keys.cpu().numpy().view(np.uint64), wk, err_msg="keys at cap %d" % mp)
        assert wm.max() >= min(mp, 3) and (wm == 0).any()


def _run(game, G, S, B, n_games, sbt0, openings=None, early=None, cap=None, resign=None, stagger=False, pool=False,
         one_call=False, evict=False, seed=SEED, set_after=None):
    """play exactly the games with local index < n_games (games_limit); returns ({uid: game dict}, raw drains,
    counters).  openings: max_plies, or None: the call is never made.  set_after = (passes, max_plies): a second set
    call in mid-run"""
    from caro_ai_amd.engine import SelfPlayEngine
    from caro_ai_amd.net_hip import HashNet
    from caro_ai_amd.resign import split_games
    hw = game.obs_shape[1] * game.obs_shape[2]
    eng = SelfPlayEngine(game, G, evaluators=[HashNet(game, device=DEV)], max_batch=B, steps_before_tau_0=sbt0,
                         seed=seed, device=DEV, searches_hint=S, stagger=stagger, stagger_recycle=(2 if pool else 1),
                         games_limit=n_games, evict=evict, node_cap=None if evict else S * B * hw + 64)
    if cap is not None:
        eng.set_playout_cap(*cap)
    if early is not None:
        eng.set_early_stop(early)
    if resign is not None:
        eng.set_resign(*resign)
    if openings is not None:
        eng.set_openings(openings)
    drains, done = [], 0
    for n in range((hw + 4) * (-(-n_games // G)) + S + 8):  # one pass = one ply per game (staggered: at most)
        if set_after is not None and n == set_after[0]:
            eng.set_openings(set_after[1])
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
    eng.close()
    assert done == n_games and c["overflows"] == 0 and c["finished"] == n_games
    games = {}
    for d in drains:
        for g in split_games(d, seed if resign is not None else None, resign[1] if resign is not None else None):
            assert g["uid"] not in games
            games[g["uid"]] = g
    return games, drains, c


_COMPOSED = {}


def _composed(d, uid, mp, S, B, sbt0, cap=None, early=None, resign_t=None, playthrough=False):
    """the oracle's game of `uid` (cached: the schedules of one test compare against the same composition)"""
    key = (tuple(sorted(d.items())), uid, mp, S, B, sbt0, cap, early, resign_t, playthrough)
    if key not in _COMPOSED:
        _COMPOSED[key] = compose_game_from(lambda: _oracle_of(d), _game_of(d), SEED, uid, uid & 1, mp, S, B, sbt0,
                                           cap=cap, early=early, resign_t=resign_t, playthrough=playthrough)
    return _COMPOSED[key]


def _assert_game(game, g, want, uid):
    states = game.from_keys(np.ascontiguousarray(g["states"]).view(np.uint64))
    assert list(states) == want["states"], uid
    np.testing.assert_array_equal(g["players"], want["players"], err_msg="players of uid %d" % uid)
    np.testing.assert_array_equal(g["pi"], want["pi"], err_msg="pi of uid %d" % uid)
    np.testing.assert_array_equal(g["z"], want["z"], err_msg="z of uid %d" % uid)
    assert g["pi"].dtype == np.float64 and g["open"].dtype == np.int16
    assert (g["open"] == want["open"]).all() and len(g["open"]) == len(want["z"]), uid
    assert (g["result"], g["steps"], g["first"]) == (want["result"], want["steps"], want["first"]), uid
    if "mb" in g:
        np.testing.assert_array_equal(g["mb"], want["mb"], err_msg="minibatches of uid %d" % uid)
    if "full" in g:
        np.testing.assert_array_equal(g["full"], want["full"], err_msg="full of uid %d" % uid)
    if g["q"] is not None:
        np.testing.assert_array_equal(g["q"], want["q"], err_msg="root Q of uid %d" % uid)


def _check_oracle(d, games, counters, G, mp, S, B, sbt0, **kw):
    """every game equals the composed one bit for bit; the sims and expansions equal the oracle's totals; at least two
    slots restarted inside the run; the openings are not trivial"""
    game = _game_of(d)
    want = [_composed(d, uid, mp, S, B, sbt0, **kw) for uid in sorted(games)]
    opens = [w["open"] for w in want]
    print("composition:", d, mp, S, B, sbt0, kw, "games", len(want), "opening plies", sorted(set(opens)),
          "plies", sum(len(w["z"]) for w in want))
    assert sum(uid >= G for uid in games) >= 2, "no slot restarted"
    assert max(opens) >= 2 and sum(o > 0 for o in opens) * 2 >= len(opens)
    assert any(w["first"] != (uid & 1) for uid, w in zip(sorted(games), want))
    for uid, w in zip(sorted(games), want):
        _assert_game(game, games[uid], w, uid)
    assert counters["sims"] == sum(w["counters"]["sims"] for w in want)
    assert counters["expansions"] == sum(w["counters"]["expansions"] for w in want)


FORMS = {"stag_recycle": dict(stagger=True), "stag_pool": dict(stagger=True, pool=True), "search_step": dict(),
         "search_move": dict(one_call=True)}


@pytest.mark.parametrize("form", list(FORMS))
def test_connect4_matches_oracle_composition(form):
    """test 2: park_and_restart (stag_recycle), k_stag_assign (stag_pool), the drain's recycle (the lock-step forms)"""
    G, S, B, N, sbt0, mp = 16, 5, 8, 32, 4, 6
    games, _, c = _run(_game_of(C4), G, S, B, N, sbt0, openings=mp, **FORMS[form])
    _check_oracle(C4, games, c, G, mp, S, B, sbt0)


@pytest.mark.parametrize("form", ["search_step", "search_move"])
def test_connect4_half_wavefront_lockstep_matches_oracle_composition(form):
    """B = 4: 32 threads per game, no fused tree kernel"""
    G, S, B, N, sbt0, mp = 12, 5, 4, 24, 4, 6
    games, _, c = _run(_game_of(C4), G, S, B, N, sbt0, openings=mp, **FORMS[form])
    _check_oracle(C4, games, c, G, mp, S, B, sbt0)


def test_mnk_5x5_staggered_pool_matches_oracle_composition():
    d = {"kind": "mnk", "n": 5, "k": 4}
    G, S, B, N, sbt0, mp = 12, 5, 8, 24, 2, 6
    games, _, c = _run(_game_of(d), G, S, B, N, sbt0, openings=mp, stagger=True, pool=True)
    _check_oracle(d, games, c, G, mp, S, B, sbt0)


def test_mnk_9x9_staggered_with_eviction_matches_oracle_composition():
    d = {"kind": "mnk", "n": 9, "k": 5}
    G, S, B, N, sbt0, mp = 6, 5, 8, 12, 2, 10
    games, _, c = _run(_game_of(d), G, S, B, N, sbt0, openings=mp, stagger=True, evict=True)
    _check_oracle(d, games, c, G, mp, S, B, sbt0)


def test_caro_7x7_multiwave_staggered_matches_oracle_composition():
    d = {"kind": "caro", "n": 7, "k": 4}
    game = _game_of(d)
    from caro_ai_amd.engine import staggered_geometry
    G, S, B, N, sbt0, mp = 8, 5, 8, 16, 3, 8
    assert staggered_geometry(game, B) and B * 64 > 64  # 8 descents x 64 lanes: k_tree_stag_mw
    games, _, c = _run(game, G, S, B, N, sbt0, openings=mp, stagger=True)
    _check_oracle(d, games, c, G, mp, S, B, sbt0)


SCHEDULES = [dict(stagger=True, pool=True), dict(one_call=True), dict()]


@pytest.mark.parametrize("kw", SCHEDULES, ids=["staggered", "search_move", "search_step"])
def test_zero_and_no_call_equal_each_other(kw):
    """test 3: set_openings(0) on an engine that never opened is today's engine, byte for byte; and the feature, on
    the same games, is not a no-op"""
    game = _game_of(C4)
    G, S, B, N, sbt0 = 16, 5, 8, 32, 4
    _, off, c0 = _run(game, G, S, B, N, sbt0, openings=None, **kw)
    _, zero, c1 = _run(game, G, S, B, N, sbt0, openings=0, **kw)
    assert c0 == c1 and len(off) == len(zero)
    for a, b in zip(off, zero):
        assert set(a) == set(b) and "open" not in a
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    _, on, c2 = _run(game, G, S, B, N, sbt0, openings=6, **kw)
    assert c2 != c0 and any((d["open"] > 0).any() for d in on)
    # switched on and off again before the first minibatch: the same tuples, with an all-zero "open" beside them
    _, back, c3 = _run(game, G, S, B, N, sbt0, openings=6, set_after=(0, 0), **kw)
    assert c3 == c0 and len(back) == len(off)
    for a, b in zip(off, back):
        assert set(b) == set(a) | {"open"} and not b["open"].any()
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k


def _tuple0(game, g):
    return (game.from_keys(np.ascontiguousarray(g["states"][:1]).view(np.uint64))[0], int(g["players"][0]),
            int(g["open"][0]))


@pytest.mark.parametrize("kw", [dict(stagger=True), dict(one_call=True)], ids=["staggered", "lockstep"])
def test_a_set_call_in_mid_run_leaves_games_in_flight_alone(kw):
    """test 4a: after three passes every first game is in flight and keeps its root (the empty board); the games that
    start later are opened"""
    game = _game_of(C4)
    G, S, B, N, sbt0, mp = 16, 5, 8, 48, 4, 6
    games, _, _ = _run(game, G, S, B, N, sbt0, openings=None, set_after=(3, mp), **kw)
    later = 0
    for uid, g in games.items():
        if uid < G:
            assert _tuple0(game, g) == (game.initial_state, uid & 1, 0), uid
        else:
            assert _tuple0(game, g) == host_opening(game, SEED, uid, uid & 1, mp), uid
            later += int(g["open"][0] > 0)
    assert later >= 8


def test_set_call_restart_reset_and_set_roots():
    """test 4b: a set call on a fresh engine opens the first games (both kinds of engine); restart keeps the setting;
    caro_reset_games with a first_player array opens from that player; caro_set_roots does not open, and a set call
    after it leaves the placed roots alone"""
    from caro_ai_amd.engine import SelfPlayEngine
    from caro_ai_amd.net_hip import HashNet
    game = _game_of(C4)
    G, mp = 64, 6

    def roots(eng):
        keys, pl, ply, uid = eng.roots()
        return list(game.from_keys(keys)), pl.tolist(), ply.tolist(), uid.tolist()

    for stagger in (False, True):
        eng = SelfPlayEngine(game, G, evaluators=[HashNet(game, device=DEV)], max_batch=8, device=DEV, searches_hint=5,
                             steps_before_tau_0=2, stagger=stagger, node_cap=5 * 8 * 42 + 64, seed=SEED)
        s, p, _, u = roots(eng)
        assert set(s) == {game.initial_state} and p == [x & 1 for x in u]
        for cap in (mp, 3, mp):  # (a second and third call re-open the fresh games under the new cap)
            eng.set_openings(cap)
            s, p, ply, u = roots(eng)
            want = [host_opening(game, SEED, x, x & 1, cap) for x in u]
            assert list(zip(s, p)) == [w[:2] for w in want] and ply == [0] * G
        assert sum(w[2] > 0 for w in want) >= G // 2
        eng.search(5, 8)
        eng.step()
        eng.restart(seed=SEED + 1)
        assert eng.openings == mp
        s, p, _, u = roots(eng)
        assert list(zip(s, p)) == [host_opening(game, SEED + 1, x, x & 1, mp)[:2] for x in u]
        if not stagger:
            fp = [(x // 2) & 1 for x in range(G)]
            eng.reset(first_players=fp)
            s, p, _, u = roots(eng)
            assert list(zip(s, p)) == [host_opening(game, SEED + 1, x, f, mp)[:2] for x, f in zip(u, fp)]
            placed = [game.move(game.initial_state, 3, 0)[0]] * G
            eng.set_roots(placed, [1] * G)
            assert roots(eng)[:2] == (placed, [1] * G)
            eng.set_openings(2)
            assert roots(eng)[:2] == (placed, [1] * G)
        eng.close()


@pytest.mark.parametrize("kw", [dict(stagger=True), dict(one_call=True)], ids=["staggered", "lockstep"])
def test_composes_with_playout_cap_and_early_stop(kw):
    """test 5a: playout cap (0.5, 2) and early stop (1), each together with max_plies = 4: the classes and the cuts are
    those of the searched ply indices"""
    G, S, B, N, sbt0, mp = 12, 6, 8, 24, 4, 4
    games, _, c = _run(_game_of(C4), G, S, B, N, sbt0, openings=mp, cap=(0.5, 2), **kw)
    _check_oracle(C4, games, c, G, mp, S, B, sbt0, cap=(0.5, 2))
    assert any(not f for g in games.values() for f in g["full"]) and any(f for g in games.values() for f in g["full"])
    games, _, c = _run(_game_of(C4), G, S, B, N, sbt0, openings=mp, early=1, **kw)
    _check_oracle(C4, games, c, G, mp, S, B, sbt0, early=1)
    assert any(m < S for g in games.values() for m in g["mb"])


@pytest.mark.parametrize("kw", [dict(stagger=True), dict(one_call=True)], ids=["staggered", "lockstep"])
def test_composes_with_resignation(kw):
    """test 5b: the threshold from the off run's q quantile, as tests/test_gpu_early_stop.py takes it; resigned games
    are prefixes of the recorded ones and equal their composition"""
    game = _game_of(C4)
    G, S, B, N, sbt0, mp, pt = 16, 6, 8, 32, 4, 4, 0.25
    off, _, c = _run(game, G, S, B, N, sbt0, openings=mp, resign=(-1.0, pt), **kw)
    _check_oracle(C4, off, c, G, mp, S, B, sbt0)
    mins = sorted(float(g["q"].min()) for g in off.values() if not g["playthrough"])
    t = float(np.nextafter(mins[len(mins) // 2 - 1], np.inf))
    on, _, _ = _run(game, G, S, B, N, sbt0, openings=mp, resign=(t, pt), **kw)
    assert _check_prefixes(off, on, t) > 0
    some = [uid for uid, b in on.items() if b["resigned"]][:4]
    assert some
    for uid in some:
        w = _composed(C4, uid, mp, S, B, sbt0, resign_t=t)
        assert w["resigned"]
        _assert_game(game, on[uid], w, uid)


def _is_successor(L, key, player, nxt):
    """connect four: `nxt` is `key` after one legal move of `player` (caro_host_move refuses a full column)"""
    k, won = (C.c_uint64 * 1)(), C.c_int()
    for a in range(7):
        k[0] = key
        if L.caro_host_move(0, 0, 0, k, a, player, C.byref(won)) == 0 and k[0] == nxt:
            return True
    return False


def test_staggered_at_1024_slots():
    """test 6: 1 024 staggered Connect4 slots, max_plies = 8, 60 launches (30 passes of 2 x 8)"""
    from caro_ai_amd.engine import SelfPlayEngine
    from caro_ai_amd.net_hip import HashNet
    from caro_ai_amd import _lib
    from caro_ai_amd.resign import split_games
    L = _lib.load()
    game = _game_of(C4)
    G, S, B, mp = 1024, 2, 8, 8
    eng = SelfPlayEngine(game, G, evaluators=[HashNet(game, device=DEV)], max_batch=B, steps_before_tau_0=4, seed=SEED,
                         device=DEV, searches_hint=S, stagger=True, stagger_recycle=1, node_cap=S * B * 42 + 64)
    eng.set_openings(mp)
    games = []
    for _ in range(60 // S):
        eng.search(S, B)
        d = eng.drain(recycle=True)
        if d["games"].shape[0]:
            games += split_games({k: v.cpu().numpy() for k, v in d.items()})
    c = eng.counters()
    eng.close()
    assert c["overflows"] == 0
    uids = np.array([g["uid"] for g in games], dtype=np.uint64)
    assert len(set(uids.tolist())) == len(uids)
    # the bound, from the host helper alone over the drained uids
    wk, wp, wm = _host_keys(game, SEED, uids, (uids & np.uint64(1)).astype(np.int32), mp)
    distinct = len({(int(k[0]), int(p)) for k, p in zip(wk, wp)})
    print("1 024 slots: %d games drained, %d distinct tuple-0 positions, opening plies mean %.2f" % (
        len(games), distinct, wm.mean()))
    assert distinct >= 900
    got = set()
    for g, k, p, m in zip(games, wk, wp, wm):
        keys = np.ascontiguousarray(g["states"]).view(np.uint64)
        assert (int(keys[0, 0]), int(g["players"][0])) == (int(k[0]), int(p)), g["uid"]
        assert (g["open"] == m).all() and g["first"] == p
        got.add((int(keys[0, 0]), int(g["players"][0])))
        for i in range(len(keys) - 1):  # every move is legal: the next root is one of the (at most seven) successors
            assert _is_successor(L, int(keys[i, 0]), int(g["players"][i]), int(keys[i + 1, 0])), (g["uid"], i)
    assert len(got) == distinct


def _shipped_net(game):
    import os
    from caro_ai_amd.lib.model import Net
    net = Net(game.obs_shape, game.action_space)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    net.load_state_dict(torch.load(os.path.join(root, "caro_ai_amd", "data", "weights", "best_026_12000.dat"),
                                   map_location="cpu"))
    return net.to(DEV).eval()


def test_self_play_reports_and_keeps_every_tuple():
    """test 7a: train.self_play / self_play_stream / play_games with openings=4, the shipped Connect4 net"""
    import collections
    from caro_ai_amd import config as cfg
    from caro_ai_amd import train
    from caro_ai_amd.lib import utils
    game = _game_of(C4)
    net = _shipped_net(game)
    S = 10

    def check(out, games):
        print({k: out[k] for k in ("open_plies_mean", "open_games")})
        assert 0.0 < out["open_plies_mean"] <= 4.0 and 0 < out["open_games"] <= games

    for stagger in (True, False):
        buf = train.DeviceReplayBuffer(game, 100000, DEV)
        out = train.self_play(game, buf, net, 64, device=DEV, seed=4, searches=S, batch=8, stagger=stagger,
                              reuse=False, openings=4)
        assert len(buf) == out["rows"] == out["steps"] + 64
        check(out, 64)
    plain = train.DeviceReplayBuffer(game, 100000, DEV)
    ref = train.self_play(game, plain, net, 64, device=DEV, seed=4, searches=S, batch=8, stagger=True, reuse=False,
                          openings=0)
    assert "open_games" not in ref and len(plain) == ref["rows"]
    buf = train.DeviceReplayBuffer(game, 100000, DEV)
    rows = 0
    # (the second call re-uses the stream and its setting; the third changes the setting on the reused stream: the rows
    # of the pass left open by the second call are taken before the set call and reach the buffer with the rest)
    for call, mp in enumerate((4, 4, 2)):
        out = train.self_play_stream(game, buf, net, 64, device=DEV, seed=4, searches=S, batch=8, openings=mp)
        assert out["engine_reused"] == (call > 0) and out["games"] >= 64
        # (the bound stays 4.0 in the third call, not its own 2: the games opened under 4 before the switch keep their
        # roots and finish inside it, so its mean mixes both settings)
        assert 0.0 < out["open_plies_mean"] <= 4.0 and 0 < out["open_games"] <= out["games"]
        rows += out["rows"]
        assert len(buf) == rows  # every tuple of every call, the carried ones included
    eng = next(iter(train._ENGINES.values()))
    assert eng.openings == 2
    train.release_engines()
    dq = collections.deque()
    res, stats = utils.play_games(game, 32, dq, net, steps_before_tau_0=cfg.STEPS_BEFORE_TAU_0, mcts_searches=S,
                                  mcts_batch_size=8, seed=4, device=DEV, return_stats=True, openings=4)
    assert len(dq) == sum(stats["steps"]) + 32
    check(stats, 32)
    with pytest.raises(ValueError):
        utils.play_games(game, 4, dq, net, net2=torch.nn.Identity(), openings=4, device=DEV)  # an arena never opens


def test_cli_opening_plies_option_runs_and_is_logged(tmp_path, monkeypatch):
    """test 7b: python -m caro_ai_amd.train --opening-plies 4 --iterations 1 runs and logs the option"""
    from caro_ai_amd import train
    rows, lines = [], []

    class Writer:
        def add_scalar(self, name, value, step):
            rows.append((name, float(value), step))

        def close(self):
            pass

    monkeypatch.setattr(train, "_writer", lambda name: Writer())
    monkeypatch.setattr("builtins.print", lambda *a, **k: lines.append(" ".join(str(x) for x in a)))
    train.main(["-n", "r", "-g", "0", "--cuda", "--games", "64", "--iterations", "1", "--saves", str(tmp_path),
                "--opening-plies", "4"])
    got = {r[0]: r[1] for r in rows}
    assert 0.0 < got["open_plies_mean"] <= 4.0 and 0 < got["open_games"] <= 64
    assert any(line.startswith("Openings: up to 4 plies") for line in lines)
