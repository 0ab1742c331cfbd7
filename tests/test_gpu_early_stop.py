"""Early stop of decided tau = 0 plies on the GPU (include/caro_hip.h, "early stop"; SelfPlayEngine.set_early_stop): the
engine's games equal the game composed ply by ply on the oracle (tests/early_stop_ref.py) in every schedule; a floor
that never fires and an engine without the call equal today's engine; the guarantee itself (same move, same tuple up
to the first cut ply); resignation and the playout cap compose with it; the staggered run at scale; the argument
checks; the training path and the train CLI.

Every engine here evaluates with the table net (HashNet), the oracle with its twin (use_synth_net), unless said
otherwise.  The parameters were fixed from the composition on the CPU alone (seed 5, uids 0 .. n-1, first player = uid & 1,
B = 8, min_minibatches = 1); its counts are in the comments at each test and are asserted from the composed games."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.early_stop_ref import compose_game, tally
from tests.test_gpu_engine import DEV, _game_of, _oracle_of
from tests.test_gpu_resign import _check_prefixes

pytestmark = pytest.mark.gpu

C4 = {"kind": "c4"}
SEED = 5


def _run(game, G, S, B, n_games, sbt0, early=1, cap=None, resign=None, stagger=False, pool=False, one_call=False,
         evict=False, seed=SEED):
    """play exactly the games with local index < n_games (games_limit); returns ({uid: game dict}, raw drains,
    counters).  early: min_minibatches, or None: the call is never made"""
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
    drains, done, evicted = [], 0, False
    for _ in range((hw + 4) * (-(-n_games // G)) + S + 8):  # one pass = one ply per game (staggered: at most)
        if evict:  # (a tree that holds fewer nodes than it ever made has dropped some: eviction is not inert here)
            evicted = evicted or bool((eng.tree_live() < eng.tree_sizes()).any())
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
    assert evicted == bool(evict)
    games = {}
    for d in drains:
        for g in split_games(d, seed if resign is not None else None, resign[1] if resign is not None else None):
            assert g["uid"] not in games
            games[g["uid"]] = g
    return games, drains, c


_COMPOSED = {}


def _composed(d, uid, S, B, sbt0, min_mb=1, cap=None, seed=SEED):
    """the oracle's game of `uid` (cached: the schedules of one test compare against the same composition)"""
    key = (tuple(sorted(d.items())), uid, S, B, sbt0, min_mb, cap, seed)
    if key not in _COMPOSED:
        _COMPOSED[key] = compose_game(lambda: _oracle_of(d), seed, uid, uid & 1, S, B, sbt0, min_mb, cap)
    return _COMPOSED[key]


def _assert_game(game, g, want, uid, q=False):
    states = game.from_keys(np.ascontiguousarray(g["states"]).view(np.uint64))
    assert list(states) == want["states"], uid
    np.testing.assert_array_equal(g["players"], want["players"], err_msg="players of uid %d" % uid)
    np.testing.assert_array_equal(g["pi"], want["pi"], err_msg="pi of uid %d" % uid)
    np.testing.assert_array_equal(g["z"], want["z"], err_msg="z of uid %d" % uid)
    np.testing.assert_array_equal(g["mb"], want["mb"], err_msg="minibatches of uid %d" % uid)
    assert g["pi"].dtype == np.float64 and g["mb"].dtype == np.int16
    assert (g["result"], g["steps"], g["first"]) == (want["result"], want["steps"], uid & 1), uid
    if q:
        np.testing.assert_array_equal(g["q"], want["q"], err_msg="root Q of uid %d" % uid)


def _check_oracle(d, games, counters, S, B, sbt0, min_mb=1, cap=None, quarter=True):
    """test 1: every game equals the composed one bit for bit; the engine's sims and expansions equal the oracle's
    totals over the same games.  Returns the composition's tally"""
    game = _game_of(d)
    want = [_composed(d, uid, S, B, sbt0, min_mb, cap) for uid in sorted(games)]
    t = tally(want)
    print("composition:", d, S, B, sbt0, min_mb, cap, t)
    # the conditions, for the composed oracle alone
    assert t["cut"] >= 1 and t["tau0"] > t["cut"]
    assert any(gw["tau0"][i] and gw["mb"][i] == gw["budget"][i] for gw in want for i in range(len(gw["mb"])))
    if quarter:
        assert 4 * t["games_cut"] >= t["games"]
    for uid, w in zip(sorted(games), want):
        _assert_game(game, games[uid], w, uid)
        if cap is not None:
            np.testing.assert_array_equal(games[uid]["full"], w["full"], err_msg="full of uid %d" % uid)
    assert counters["sims"] == sum(w["counters"]["sims"] for w in want)
    assert counters["expansions"] == sum(w["counters"]["expansions"] for w in want)
    assert counters["sims"] == (t["budget"] - t["saved"]) * B
    return t


FORMS = {"stag_recycle": dict(stagger=True), "stag_pool": dict(stagger=True, pool=True), "search_step": dict(),
         "search_move": dict(one_call=True)}


@pytest.mark.parametrize("form", list(FORMS))
def test_connect4_matches_oracle_composition(form):
    # composition: 40 games, 30 with a cut ply, 548 plies, 388 at tau = 0, 30 cut, 46 of 3 288 minibatches saved
    G, S, B, N, sbt0 = 16, 6, 8, 40, 4
    games, _, c = _run(_game_of(C4), G, S, B, N, sbt0, **FORMS[form])
    t = _check_oracle(C4, games, c, S, B, sbt0)
    assert (t["games_cut"], t["plies"], t["tau0"], t["cut"], t["saved"], t["budget"]) == (30, 548, 388, 30, 46, 3288)


def test_connect4_deeper_budget_and_floor():
    # S = 10: 16 games, all with a cut ply, 215 plies, 151 at tau = 0, 18 cut, 52 of 2 150 saved; the same with floor 3
    G, S, B, N, sbt0 = 16, 10, 8, 16, 4
    for min_mb in (1, 3):
        games, _, c = _run(_game_of(C4), G, S, B, N, sbt0, early=min_mb, stagger=True)
        t = _check_oracle(C4, games, c, S, B, sbt0, min_mb)
        assert (t["cut"], t["saved"], t["budget"]) == (18, 52, 2150)


@pytest.mark.parametrize("form", ["search_step", "search_move"])
def test_connect4_half_wavefront_lockstep_matches_oracle_composition(form):
    """B = 4: 32 threads per game, no fused tree kernel -- caro_search_batch runs k_select / k_encode / k_expand_backup
    and hands the select its budget.  Composition: 24 games, 23 with a cut ply, 309 plies, 213 at tau = 0, 24 cut, 54 of
    2 472 minibatches saved"""
    G, S, B, N, sbt0 = 12, 8, 4, 24, 4
    games, _, c = _run(_game_of(C4), G, S, B, N, sbt0, **FORMS[form])
    t = _check_oracle(C4, games, c, S, B, sbt0)
    assert (t["games_cut"], t["cut"], t["saved"], t["budget"]) == (23, 24, 54, 2472)


def test_caro_7x7_multiwave_staggered_matches_oracle_composition():
    # composition: 24 games, 17 with a cut ply, 465 plies, 393 at tau = 0, 17 cut, 28 of 2 790 saved
    d = {"kind": "caro", "n": 7, "k": 4}
    game = _game_of(d)
    from caro_ai_amd.engine import staggered_geometry
    G, S, B, N, sbt0 = 12, 6, 8, 24, 3
    assert staggered_geometry(game, B) and B * 64 > 64  # 8 descents x 64 lanes: k_tree_stag_mw
    games, _, c = _run(game, G, S, B, N, sbt0, stagger=True)
    t = _check_oracle(d, games, c, S, B, sbt0)
    assert (t["games_cut"], t["cut"], t["saved"]) == (17, 17, 28)


@pytest.mark.parametrize("form", ["stag_pool", "search_move"])
def test_mnk_5x5_matches_oracle_composition(form):
    # composition: 24 games, 18 with a cut ply, 347 plies, 299 at tau = 0, 19 cut, 31 of 2 082 saved
    d = {"kind": "mnk", "n": 5, "k": 4}
    G, S, B, N, sbt0 = 12, 6, 8, 24, 2
    games, _, c = _run(_game_of(d), G, S, B, N, sbt0, **FORMS[form])
    t = _check_oracle(d, games, c, S, B, sbt0)
    assert (t["games_cut"], t["cut"], t["saved"]) == (18, 19, 31)


@pytest.mark.parametrize("form", ["stag_evict", "search_move"])
def test_mnk_9x9_two_actions_per_lane_matches_oracle_composition(form):
    """9 x 9 k = 5: 81 actions on 64 lanes, two per lane (APL = 2), one wavefront per descent; the staggered run with
    eviction on (_run asserts that trees did drop nodes).  Composition: 12 games, 7 with a cut ply, 458 plies, 434 at tau = 0, 7 cut, 12 of 2 748 minibatches
    saved"""
    d = {"kind": "mnk", "n": 9, "k": 5}
    G, S, B, N, sbt0 = 12, 6, 8, 12, 2
    kw = dict(stagger=True, evict=True) if form == "stag_evict" else dict(one_call=True)
    games, _, c = _run(_game_of(d), G, S, B, N, sbt0, **kw)
    t = _check_oracle(d, games, c, S, B, sbt0)
    assert (t["games_cut"], t["cut"], t["saved"], t["budget"]) == (7, 7, 12, 2748)


SCHEDULES = [dict(stagger=True, pool=True), dict(one_call=True), dict()]


@pytest.mark.parametrize("kw", SCHEDULES, ids=["staggered", "search_move", "search_step"])
def test_a_floor_that_never_fires_and_no_call_equal_todays_engine(kw):
    """test 2: min_minibatches > M - 2 leaves every tuple and the counters byte-identical to an engine on which the call
    was never made; only "mb" is added, every count M"""
    game = _game_of(C4)
    G, S, B, N, sbt0 = 16, 6, 8, 32, 4
    _, off, c0 = _run(game, G, S, B, N, sbt0, early=None, **kw)
    _, on, c1 = _run(game, G, S, B, N, sbt0, early=S - 1, **kw)
    assert c0 == c1 and len(off) == len(on)
    for a, b in zip(off, on):
        assert set(b) == set(a) | {"mb"} and "mb" not in a
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
        assert b["mb"].dtype == np.int16 and b["mb"].shape == b["z"].shape and (b["mb"] == S).all()
    # and the feature, on the same games, is not a no-op
    _, cut, c2 = _run(game, G, S, B, N, sbt0, early=1, **kw)
    assert c2["sims"] < c0["sims"] and any((d["mb"] < S).any() for d in cut)


@pytest.mark.parametrize("kw", [dict(one_call=True), dict()], ids=["search_move", "search_step"])
def test_the_guarantee_up_to_the_first_cut_ply(kw):
    """test 3: lock-step, an engine with the feature and one without, same seed: for every game the plies up to and
    including its first cut ply carry the same state, pi and (so the next state says) action"""
    game = _game_of(C4)
    G, S, B, N, sbt0 = 16, 6, 8, 40, 4
    off, _, _ = _run(game, G, S, B, N, sbt0, early=None, **kw)
    on, _, _ = _run(game, G, S, B, N, sbt0, early=1, **kw)
    n_cut = n_uncut_tau0 = 0
    for uid, b in on.items():
        a = off[uid]
        cut = np.flatnonzero(b["mb"] < S)
        n = int(cut[0]) + 1 if len(cut) else len(b["mb"])
        n_cut += len(cut)
        n_uncut_tau0 += int(((b["mb"] == S) & (np.arange(len(b["mb"])) >= sbt0)).sum())
        assert (cut >= sbt0).all() and (b["mb"][cut] >= 2).all() and (b["mb"][cut] <= S - 1).all()
        assert len(a["z"]) >= n
        for k in ("states", "players", "pi"):
            np.testing.assert_array_equal(a[k][:n], b[k][:n], err_msg="%s of uid %d" % (k, uid))
        # the action of ply n - 1: the state that follows it (or, if the game ended there, its record)
        if n < len(b["z"]):
            assert len(a["z"]) > n
            np.testing.assert_array_equal(a["states"][n], b["states"][n], err_msg="action of uid %d" % uid)
        elif not len(cut):
            assert (a["result"], a["steps"]) == (b["result"], b["steps"]), uid
    assert n_cut >= 1 and n_uncut_tau0 >= 1


def test_composes_with_the_playout_cap():
    """test 4a: M = fast on fast plies (composition, 24 games at (0.5, 5), S = 10: 17 games with a cut ply, 17 cut of
    191 tau = 0 plies, 39 of 2 055 minibatches saved)"""
    G, S, B, N, sbt0, cap = 12, 10, 8, 24, 4, (0.5, 5)
    for kw in (dict(stagger=True), dict(one_call=True)):
        games, _, c = _run(_game_of(C4), G, S, B, N, sbt0, cap=cap, **kw)
        t = _check_oracle(C4, games, c, S, B, sbt0, cap=cap)
        assert (t["games_cut"], t["cut"], t["saved"], t["budget"]) == (17, 17, 39, 2055)


@pytest.mark.parametrize("kw", [dict(stagger=True), dict(one_call=True)], ids=["staggered", "lockstep"])
def test_composes_with_resignation(kw):
    """test 4b: the root Q recorded at every ply, cut plies included, is the oracle's Q of the first-max-N edge on the cut
    tree; with a threshold, resigned games are prefixes of the same games without one (the resign tests' check)"""
    game = _game_of(C4)
    G, S, B, N, sbt0, pt = 16, 6, 8, 40, 4, 0.25
    off, _, _ = _run(game, G, S, B, N, sbt0, resign=(-1.0, pt), **kw)
    n_cut = 0
    for uid, g in off.items():
        w = _composed(C4, uid, S, B, sbt0)
        _assert_game(game, g, w, uid, q=True)
        n_cut += sum(m < S for m in w["mb"])
    assert n_cut >= 1
    mins = sorted(float(g["q"].min()) for g in off.values() if not g["playthrough"])
    t = float(np.nextafter(mins[len(mins) // 2 - 1], np.inf))
    on, _, _ = _run(game, G, S, B, N, sbt0, resign=(t, pt), **kw)
    assert _check_prefixes(off, on, t) > 0
    for uid, b in on.items():
        np.testing.assert_array_equal(off[uid]["mb"][:len(b["mb"])], b["mb"], err_msg="mb of uid %d" % uid)
    # and the composition with the threshold: a resigned game is the oracle's
    some = [uid for uid, b in on.items() if b["resigned"]][:4]
    assert some
    for uid in some:
        w = compose_game(lambda: _oracle_of(C4), SEED, uid, uid & 1, S, B, sbt0, resign_t=t)
        assert w["resigned"]
        _assert_game(game, on[uid], w, uid, q=True)


def test_lockstep_search_calls_decide_each_for_themselves():
    """Lock-step, two caro_search_batch calls on the same roots before the ply: the second call starts undecided at its
    minibatch 0 (m = 0 is never decided, so every live game selects at least minibatches 0 and 1 of it), whatever the
    first call decided; the ply records the count of its last call"""
    from caro_ai_amd.engine import SelfPlayEngine
    from caro_ai_amd.net_hip import HashNet
    game = _game_of(C4)
    G, S, B = 64, 6, 8
    eng = SelfPlayEngine(game, G, evaluators=[HashNet(game, device=DEV)], max_batch=B, steps_before_tau_0=2, seed=SEED,
                         device=DEV, searches_hint=S, node_cap=2 * S * B * 42 + 64)
    eng.set_early_stop(1)
    cut_first = cut_second = 0
    mbs = []
    for _ in range(12):
        live = eng.live_games()
        if not live:
            break
        c0 = eng.counters()["sims"]
        eng.search(S, B)
        c1 = eng.counters()["sims"]
        eng.search(S, B)
        c2 = eng.counters()["sims"]
        assert (c1 - c0) % B == 0 and 2 * live * B <= c1 - c0 <= S * live * B
        assert 2 * live * B <= c2 - c1 <= S * live * B, "a game decided in the first call selected nothing in the second"
        cut_first += S * live - (c1 - c0) // B
        cut_second += S * live - (c2 - c1) // B
        eng.step()
        d = eng.drain(recycle=False)
        if d["games"].shape[0]:
            mbs.append(d["mb"].cpu().numpy())
    c = eng.counters()
    eng.close()
    assert c["overflows"] == 0
    assert cut_first >= 1 and cut_second >= 1   # (both calls cut somewhere: the test is not vacuous)
    mbs = np.concatenate(mbs)
    assert (mbs >= 2).all() and (mbs <= S).all() and (mbs < S).any()


def test_fit_runs_its_stop_callback_with_early_stop(monkeypatch):
    """train.fit with early_stop= past the replay threshold: the iteration trains, the caller's stop(history) callback
    is called and ends the loop, and the history holds the counters"""
    from caro_ai_amd import config as cfg
    from caro_ai_amd import train
    from caro_ai_amd.lib.model import Net
    monkeypatch.setattr(cfg, "MIN_REPLAY_TO_TRAIN", 256)
    game = _game_of(C4)
    torch.manual_seed(0)
    net = Net(game.obs_shape, game.action_space).to(DEV)
    calls = []

    def stop(h):
        calls.append(len(h["loss_total"]))
        return len(calls) >= 2

    h = train.fit(game, net, DEV, games=64, iterations=6, sample_seed=3, log=None, stop=stop, reference_evaluate=False,
                  early_stop=1)
    train.release_engines()
    assert calls == [1, 2] or (len(calls) == 2 and calls[0] >= 1), calls
    assert len(h["early_stop"]) == 2 and len(h["loss_total"]) >= 1
    for e in h["early_stop"]:
        assert 0 < e["stop_plies"] <= e["stop_tau0_plies"] and 0.0 < e["stop_share"] <= 1.0


def _scale_run(early, passes):
    from caro_ai_amd.engine import SelfPlayEngine
    from caro_ai_amd.net_hip import HashNet
    from caro_ai_amd.resign import split_games
    game = _game_of(C4)
    G, S, B, sbt0 = 1024, 25, 8, 4
    eng = SelfPlayEngine(game, G, evaluators=[HashNet(game, device=DEV)], max_batch=B, steps_before_tau_0=sbt0,
                         seed=SEED, device=DEV, searches_hint=S, stagger=True, stagger_recycle=1, node_cap=S * B * 42 + 64)
    if early is not None:
        eng.set_early_stop(early)
    games, finished, n = {}, 0, 0
    while (finished < 2048) if passes is None else (n < passes):
        eng.search(S, B)
        n += 1
        d = eng.drain(recycle=True)
        finished += int(d["games"].shape[0])
        if d["games"].shape[0] and early is not None:
            uids = d["games"][:, 0].cpu().numpy()
            if ((uids % 97 == 0) & (uids < 3 * G)).any():   # sampled games of the first three slot generations
                for g in split_games({k: v.cpu().numpy() for k, v in d.items()}):
                    if g["uid"] % 97 == 0 and g["uid"] < 3 * G:
                        games[g["uid"]] = g
        assert n < 400
    c = eng.counters()
    pending = eng.pending_leaves()
    eng.close()
    return games, finished, n, c, pending


def test_staggered_at_1024_slots():
    """test 5: 1 024 Connect4 slots, 25 x 8, until >= 2 048 games have finished"""
    S, B, sbt0 = 25, 8, 4
    games, finished, passes, c, pending = _scale_run(1, None)
    assert c["overflows"] == 0
    assert c["sims"] == c["expansions"] + c["terminals"] + c["dropped"] + pending
    assert len(games) >= 12
    game = _game_of(C4)
    want = []
    for uid in sorted(games):
        w = compose_game(lambda: _oracle_of(C4), SEED, uid, uid & 1, S, B, sbt0)
        _assert_game(game, games[uid], w, uid)
        want.append(w)
    t = tally(want)
    print("composition at 25 x 8:", t)
    assert t["cut"] >= 1 and t["tau0"] > t["cut"]
    _, finished0, _, c0, _ = _scale_run(None, passes)
    print("early stop: %d games, %.3f minibatches per ply; off: %d games, %.3f" % (
        finished, c["sims"] / B / c["plies"], finished0, c0["sims"] / B / c0["plies"]))
    assert c["sims"] / c["plies"] < c0["sims"] / c0["plies"]
    assert finished >= finished0


def test_argument_checks_states_and_restart():
    """test 6a: 0 / negative -> CARO_E_INVAL and ValueError; the drain's minibatches_dev before the set call and the set
    call with a select or a drain pending -> CARO_E_STATE; the setting survives restart"""
    from caro_ai_amd import _lib
    from caro_ai_amd.engine import SelfPlayEngine
    from caro_ai_amd.net_hip import HashNet
    from tests.synth_net import SynthNet
    L = _lib.load()
    game = _game_of(C4)
    for stagger in (False, True):
        eng = SelfPlayEngine(game, 8, evaluators=[HashNet(game, device=DEV)], max_batch=8, device=DEV, searches_hint=6,
                             steps_before_tau_0=2, stagger=stagger, node_cap=6 * 8 * 42 + 64, seed=SEED)
        for bad in (0, -1):
            assert L.caro_engine_set_early_stop(eng.h, bad) == -22
            with pytest.raises(ValueError):
                eng.set_early_stop(bad)
        cap = 8 * 42
        bufs = [torch.zeros(n, dtype=dt, device=DEV) for n, dt in
                [(cap, torch.int64), (cap, torch.int32), (cap * 7, torch.float64), (cap, torch.int32),
                 (32, torch.int64), (cap, torch.int16)]]
        p = [C.c_void_p(b.data_ptr()) for b in bufs]
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ex = _lib.CaroDrainExtra(None, None, p[5])

        def begin(extra):
            if stagger:
                return L.caro_drain_parked_begin_ex(eng.h, cap, p[0], p[1], p[2], p[3], p[4], extra, st)
            return L.caro_drain_tuples_begin_ex(eng.h, cap, p[0], p[1], p[2], p[3], p[4], 1, extra, st)

        assert begin(C.byref(ex)) == -71
        assert eng.early_stop is None
        eng.set_early_stop(3)
        eng.set_early_stop(1)
        assert eng.early_stop == 1
        assert begin(C.byref(ex)) == 0        # a drain is pending
        assert L.caro_engine_set_early_stop(eng.h, 2) == -71
        nt, ng = C.c_int64(0), C.c_int64(0)
        assert L.caro_drain_tuples_end(eng.h, C.addressof(nt), C.addressof(ng)) == 0
        assert begin(None) == 0               # extra = NULL: a plain drain
        assert L.caro_drain_tuples_end(eng.h, C.addressof(nt), C.addressof(ng)) == 0

        def play(n):
            out = []
            for _ in range(200):
                if stagger:
                    eng.search(6, 8)
                else:
                    eng.search_step(6, 8)
                d = eng.drain(recycle=True)
                out += [d["mb"].cpu().numpy()] if d["games"].shape[0] else []
                if sum(len(x) for x in out) >= n:
                    return np.concatenate(out)
            raise AssertionError("no games finished")

        a = play(150)
        eng.restart()
        assert eng.early_stop == 1
        b = play(150)
        assert (a < 6).any() and (a >= 2).all() and (a <= 6).all()
        np.testing.assert_array_equal(a, b[:len(a)])   # the same games, cut at the same plies
        eng.close()
    # a pending caro_select (the step-wise form: a host-evaluated net)
    eng = SelfPlayEngine(game, 8, evaluators=[SynthNet(84, 7, DEV)], max_batch=8, device=DEV, searches_hint=4,
                         node_cap=4 * 8 * 42 + 64)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.caro_select(eng.h, 8, 0, None, C.c_void_p(eng.planes.data_ptr()), C.c_void_p(eng.leaf_keys.data_ptr()),
                         st) == 0
    assert L.caro_engine_set_early_stop(eng.h, 1) == -71
    with pytest.raises(_lib.CaroError):
        eng.set_early_stop(1)
    assert L.caro_select_cancel(eng.h) == 0
    eng.set_early_stop(1)
    eng.close()


def test_self_play_reports_and_keeps_every_tuple():
    """test 6b: train.self_play / self_play_stream / play_games with early_stop=, the shipped Connect4 net: every tuple
    reaches the replay buffer, the counters are reported"""
    import collections
    import os
    from caro_ai_amd import config as cfg
    from caro_ai_amd import train
    from caro_ai_amd.lib import utils
    from caro_ai_amd.lib.model import Net
    game = _game_of(C4)
    net = Net(game.obs_shape, game.action_space)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    net.load_state_dict(torch.load(os.path.join(root, "caro_ai_amd", "data", "weights", "best_026_12000.dat"),
                                   map_location="cpu"))
    net = net.to(DEV).eval()
    S = 10

    def check(out, rows, games):
        print({k: out[k] for k in ("stop_plies", "stop_tau0_plies", "stop_minibatches_saved")})
        assert 0 < out["stop_plies"] <= out["stop_tau0_plies"] < rows
        assert out["stop_plies"] <= out["stop_minibatches_saved"] <= out["stop_plies"] * (S - 2)

    for stagger in (True, False):
        buf = train.DeviceReplayBuffer(game, 100000, DEV)
        out = train.self_play(game, buf, net, 64, device=DEV, seed=4, searches=S, batch=8, stagger=stagger,
                              reuse=False, early_stop=1)
        assert len(buf) == out["rows"] == out["steps"] + 64
        check(out, out["rows"], 64)
        plain = train.DeviceReplayBuffer(game, 100000, DEV)
        ref = train.self_play(game, plain, net, 64, device=DEV, seed=4, searches=S, batch=8, stagger=stagger,
                              reuse=False)
        assert "stop_plies" not in ref and len(plain) == ref["rows"]
    buf = train.DeviceReplayBuffer(game, 100000, DEV)
    out = train.self_play_stream(game, buf, net, 64, device=DEV, seed=4, searches=S, batch=8, early_stop=2)
    assert len(buf) == out["rows"]
    check(out, out["rows"], 64)
    train.release_engines()
    dq = collections.deque()
    res, stats = utils.play_games(game, 32, dq, net, steps_before_tau_0=cfg.STEPS_BEFORE_TAU_0, mcts_searches=S,
                                  mcts_batch_size=8, seed=4, device=DEV, return_stats=True, early_stop=1)
    assert len(dq) == sum(stats["steps"]) + 32
    check(stats, len(dq), 32)


def test_cli_early_stop_option_logs_the_counters(tmp_path, monkeypatch):
    """test 6c: python -m caro_ai_amd.train --early-stop runs and logs the counters"""
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
                "--early-stop"])
    got = {r[0]: r[1] for r in rows}
    assert {"stop_share", "stop_minibatches_saved"} <= set(got)
    assert 0.0 < got["stop_share"] <= 1.0 and got["stop_minibatches_saved"] >= 1
    assert any(line.startswith("Early stop:") for line in lines)
