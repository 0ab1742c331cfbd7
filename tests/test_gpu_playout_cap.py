"""Playout cap randomization on the GPU (include/caro_hip.h, "playout cap randomization"; SelfPlayEngine.set_playout_cap):
the engine's games equal the reference game composed ply by ply on the oracle with the rule's per-ply search count, in
every schedule; the degenerate settings equal plain engines; resignation composes with it; fewer simulations per ply
buy more finished games; the argument checks; the training path and the train CLI.

Every engine here evaluates with the table net (HashNet), the oracle with its twin (use_synth_net)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests.test_gpu_engine import DEV, _game_of, _oracle_of
from tests.test_gpu_resign import _check_prefixes

pytestmark = pytest.mark.gpu

C4 = {"kind": "c4"}
SBT0 = 10


def _run(game, G, S, B, n_games, seed, cap=None, resign=None, stagger=False, pool=False, one_call=False, evict=False):
    """play exactly the games with local index < n_games (games_limit); returns ({uid: game dict}, raw drains,
    counters).  Game dicts are resign.split_games' (ply 0 first), with "full" when the cap is on."""
    from caro_ai_amd.engine import SelfPlayEngine
    from caro_ai_amd.net_hip import HashNet
    from caro_ai_amd.resign import split_games
    hw = game.obs_shape[1] * game.obs_shape[2]
    eng = SelfPlayEngine(game, G, evaluators=[HashNet(game, device=DEV)], max_batch=B, steps_before_tau_0=SBT0,
                         seed=seed, device=DEV, searches_hint=S, stagger=stagger, stagger_recycle=(2 if pool else 1),
                         games_limit=n_games, evict=evict, node_cap=None if evict else S * B * hw + 64)
    if cap is not None:
        eng.set_playout_cap(*cap)
    if resign is not None:
        eng.set_resign(*resign)
    drains, done = [], 0
    for _ in range((hw + 4) * (-(-n_games // G)) + S + 8):  # one pass = one ply per game (staggered: at most)
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


def _oracle_game(d, o, seed, uid, first, S, B, cap):
    """the reference's play_game (oracle/caro_oracle.c oracle_play_game) with the rule's search count per ply:
    ply i runs S minibatches if caro_host_cap_uniform(seed, uid, i) < p_full, else min(fast, S)"""
    from caro_ai_amd import _lib
    from oracle.oracle import move_uniform, sample_index
    L = _lib.load()
    p_full, fast = cap
    o.set_stream(seed, uid)
    s, player, step, tau = o.initial_state, first, 0, 1 if SBT0 > 0 else 0
    states, players, pis, flags = [], [], [], []
    while True:
        i = len(states)
        full = L.caro_host_cap_uniform(seed, uid, i) < p_full
        o.search_batch(S if full else min(fast, S), B, s, player, ply=i)
        pi = o.get_policy(s, tau)
        states.append(s)
        players.append(player)
        pis.append(pi)
        flags.append(full)
        a = sample_index(pi, move_uniform(seed, uid, i))
        s, won = o.move(s, a, player)
        if won:
            result, r = (1 if player == 0 else -1), 1
            break
        player = 1 - player
        if not len(o.possible_moves(s)):
            result, r = 0, 0
            break
        step += 1
        if step >= SBT0:
            tau = 0
    z = [r if (len(states) - 1 - j) % 2 == 0 else -r for j in range(len(states))]
    return {"states": states, "players": players, "pi": np.array(pis), "full": flags, "z": z, "result": result,
            "steps": step}


def _check_oracle(d, games, counters, seed, S, B, cap):
    """test 1: every game equals the oracle-composed one bit for bit; the engine's sims and expansions equal the
    oracle's totals over the same games"""
    game = _game_of(d)
    sims = expansions = 0
    n_fast = 0
    for uid in sorted(games):
        g = games[uid]
        o = _oracle_of(d)
        o.use_synth_net()
        want = _oracle_game(d, o, seed, uid, g["first"], S, B, cap)
        states = game.from_keys(np.ascontiguousarray(g["states"]).view(np.uint64))
        assert list(states) == want["states"], uid
        np.testing.assert_array_equal(g["players"], want["players"], err_msg="players of uid %d" % uid)
        np.testing.assert_array_equal(g["pi"], want["pi"], err_msg="pi of uid %d" % uid)
        np.testing.assert_array_equal(g["z"], want["z"], err_msg="z of uid %d" % uid)
        np.testing.assert_array_equal(g["full"], want["full"], err_msg="full of uid %d" % uid)
        assert (g["result"], g["steps"]) == (want["result"], want["steps"]), uid
        n_fast += len(want["full"]) - sum(want["full"])
        oc = o.counters()
        sims += oc["sims"]
        expansions += oc["expansions"]
    assert counters["sims"] == sims and counters["expansions"] == expansions
    assert n_fast > 0 and n_fast < sum(len(g["z"]) for g in games.values())


@pytest.mark.parametrize("form", ["stag_recycle", "stag_pool", "search_step", "search_move"])
def test_connect4_matches_oracle_composition(form):
    game = _game_of(C4)
    G, S, B, N, seed, cap = 16, 6, 8, 40, 5, (0.4, 2)
    kw = {"stag_recycle": dict(stagger=True), "stag_pool": dict(stagger=True, pool=True),
          "search_step": dict(), "search_move": dict(one_call=True)}[form]
    games, _, c = _run(game, G, S, B, N, seed, cap=cap, **kw)
    _check_oracle(C4, games, c, seed, S, B, cap)


def test_caro_7x7_staggered_matches_oracle_composition():
    d = {"kind": "caro", "n": 7, "k": 4}
    game = _game_of(d)
    from caro_ai_amd.engine import staggered_geometry
    G, S, B, N, seed, cap = 16, 4, 8, 24, 9, (0.3, 2)
    assert staggered_geometry(game, B)
    games, _, c = _run(game, G, S, B, N, seed, cap=cap, stagger=True)
    _check_oracle(d, games, c, seed, S, B, cap)


@pytest.mark.parametrize("stagger", [False, True])
def test_gomoku15_multiwave_with_eviction_matches_oracle_composition(stagger):
    """15 x 15 k = 5 at 8 descents per minibatch: several wavefronts per game -- k_tree_stag_mw, and k_tree_mw with the
    ply in the closing launch (caro_search_move) -- with eviction on"""
    d = {"kind": "mnk", "n": 15, "k": 5}
    game = _game_of(d)
    G, S, B, N, seed, cap = 12, 3, 8, 12, 3, (0.5, 2)
    kw = dict(stagger=True) if stagger else dict(one_call=True)
    games, _, c = _run(game, G, S, B, N, seed, cap=cap, evict=True, **kw)
    _check_oracle(d, games, c, seed, S, B, cap)


SCHEDULES = [dict(stagger=True, pool=True), dict(one_call=True)]


@pytest.mark.parametrize("kw", SCHEDULES, ids=["staggered", "lockstep"])
def test_all_fast_equals_a_plain_engine_at_the_fast_count(kw):
    """test 2a: p_full = 0, fast = f on an engine of S = 25 plays, uid for uid, the games of a plain engine of S = f"""
    game = _game_of(C4)
    G, B, N, seed, f = 16, 8, 32, 13, 3
    cap_games, _, _ = _run(game, G, 25, B, N, seed, cap=(0.0, f), **kw)
    plain, _, _ = _run(game, G, f, B, N, seed, **kw)
    assert sorted(cap_games) == sorted(plain)
    for uid, a in plain.items():
        b = cap_games[uid]
        assert not b["full"].any() and "full" not in a
        for k in ("states", "players", "pi", "z"):
            np.testing.assert_array_equal(a[k], b[k], err_msg="%s of uid %d" % (k, uid))
        assert (a["result"], a["steps"], a["first"]) == (b["result"], b["steps"], b["first"]), uid


@pytest.mark.parametrize("kw", SCHEDULES, ids=["staggered", "lockstep"])
@pytest.mark.parametrize("setting", ["p_full_1", "fast_eq_S"])
def test_degenerate_settings_equal_the_cap_off(kw, setting):
    """test 2b / 2c: p_full = 1 (every flag 1) and fast = S (random flags) leave every tuple and the counters
    byte-identical to an engine without the cap; only "full" is added to the drain"""
    game = _game_of(C4)
    G, S, B, N, seed = 16, 5, 8, 32, 17
    cap = (1.0, 2) if setting == "p_full_1" else (0.5, S)
    _, off, c0 = _run(game, G, S, B, N, seed, **kw)
    _, on, c1 = _run(game, G, S, B, N, seed, cap=cap, **kw)
    assert c0 == c1
    assert len(off) == len(on)
    flags = []
    for a, b in zip(off, on):
        assert set(b) == set(a) | {"full"} and "full" not in a
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
        assert b["full"].dtype == np.bool_ and b["full"].shape == b["z"].shape
        flags.append(b["full"])
    flags = np.concatenate(flags)
    if setting == "p_full_1":
        assert flags.all()
    else:
        assert 0.3 < flags.mean() < 0.7


@pytest.mark.parametrize("kw", [dict(stagger=True), dict(one_call=True)], ids=["staggered", "lockstep"])
def test_resigned_games_are_prefixes_under_the_cap(kw):
    """test 3: with the cap and resignation on, every resigned game is the prefix of the same uid under the cap alone
    (resignation applies at fast and full plies alike)"""
    game = _game_of(C4)
    G, S, B, N, seed, cap, pt = 32, 6, 8, 64, 5, (0.5, 2), 0.25
    off, _, _ = _run(game, G, S, B, N, seed, cap=cap, resign=(-1.0, pt), **kw)
    mins = sorted(float(g["q"].min()) for g in off.values() if not g["playthrough"])
    t = float(np.nextafter(mins[len(mins) // 2 - 1], np.inf))
    on, _, _ = _run(game, G, S, B, N, seed, cap=cap, resign=(t, pt), **kw)
    assert _check_prefixes(off, on, t) > 0
    for uid, b in on.items():
        np.testing.assert_array_equal(off[uid]["full"][:len(b["full"])], b["full"], err_msg="full of uid %d" % uid)


def _stream_run(cap, calls=12):
    """staggered connect four, slots restart in-kernel, the same number of launches with and without the cap"""
    from caro_ai_amd.engine import SelfPlayEngine
    from caro_ai_amd.net_hip import HashNet
    game = _game_of(C4)
    G, S, B = 64, 25, 8
    eng = SelfPlayEngine(game, G, evaluators=[HashNet(game, device=DEV)], max_batch=B, steps_before_tau_0=SBT0, seed=3,
                         device=DEV, searches_hint=S, stagger=True, stagger_recycle=1, node_cap=S * B * 42 + 64)
    if cap is not None:
        eng.set_playout_cap(*cap)
    games = 0
    for _ in range(calls):
        eng.search(S, B)  # S launches
        games += int(eng.drain(recycle=True)["games"].shape[0])
    c = eng.counters()
    eng.close()
    assert c["overflows"] == 0
    return games, c


def test_throughput_is_real_and_deterministic():
    """test 4: the same launches finish more games with the cap at (0.25, 5), at fewer simulations per ply; the same
    run twice gives the same counters"""
    g_off, c_off = _stream_run(None)
    g_on, c_on = _stream_run((0.25, 5))
    assert g_on > g_off, (g_on, g_off)
    assert c_on["sims"] / c_on["plies"] < c_off["sims"] / c_off["plies"]
    assert c_on["plies"] > c_off["plies"]
    g2, c2 = _stream_run((0.25, 5))
    assert (g2, c2) == (g_on, c_on)


def test_argument_checks_and_states():
    """test 5: p_full NaN / -0.1 / 1.1, fast 1, fast > stagger -> CARO_E_INVAL and ValueError; an _x drain with
    full_dev before the set call and the set call with a select pending -> CARO_E_STATE"""
    from caro_ai_amd import _lib
    from caro_ai_amd.engine import SelfPlayEngine
    from caro_ai_amd.net_hip import HashNet
    from tests.synth_net import SynthNet
    L = _lib.load()
    game = _game_of(C4)
    for stagger in (False, True):
        eng = SelfPlayEngine(game, 8, evaluators=[HashNet(game, device=DEV)], max_batch=8, device=DEV, searches_hint=4,
                             stagger=stagger, node_cap=4 * 8 * 42 + 64)
        bad = [(math.nan, 2), (-0.1, 2), (1.1, 2), (0.5, 1)] + ([(0.5, 5)] if stagger else [])
        for p, f in bad:
            assert L.caro_engine_set_playout_cap(eng.h, p, f) == -22, (p, f)
            with pytest.raises(ValueError):
                eng.set_playout_cap(p, f)
        cap = 8 * 42
        bufs = [torch.zeros(n, dtype=dt, device=DEV) for n, dt in
                [(cap, torch.int64), (cap, torch.int32), (cap * 7, torch.float64), (cap, torch.int32),
                 (32, torch.int64), (cap, torch.uint8)]]
        p = [C.c_void_p(b.data_ptr()) for b in bufs]
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if stagger:
            rc = L.caro_drain_parked_begin_x(eng.h, cap, p[0], p[1], p[2], p[3], p[4], None, p[5], st)
        else:
            rc = L.caro_drain_tuples_begin_x(eng.h, cap, p[0], p[1], p[2], p[3], p[4], 1, None, p[5], st)
        assert rc == -71
        assert eng.playout_cap is None
        eng.set_playout_cap(0.0, 4 if stagger else 50)
        eng.set_playout_cap(1.0, 2)
        assert eng.playout_cap == (1.0, 2)
        eng.close()
    # a pending caro_select (the step-wise form: a host-evaluated net)
    eng = SelfPlayEngine(game, 8, evaluators=[SynthNet(84, 7, DEV)], max_batch=8, device=DEV, searches_hint=4,
                         node_cap=4 * 8 * 42 + 64)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.caro_select(eng.h, 8, 0, None, C.c_void_p(eng.planes.data_ptr()), C.c_void_p(eng.leaf_keys.data_ptr()),
                         st) == 0
    assert L.caro_engine_set_playout_cap(eng.h, 0.5, 2) == -71
    with pytest.raises(_lib.CaroError):
        eng.set_playout_cap(0.5, 2)
    assert L.caro_select_cancel(eng.h) == 0
    eng.set_playout_cap(0.5, 2)
    eng.close()


def test_self_play_puts_only_full_rows_into_the_replay_buffer():
    """test 6a: train.self_play with playout_cap: the replay buffer gets exactly the full plies' rows, and the result
    holds both shares"""
    from caro_ai_amd import train
    from caro_ai_amd.lib.model import Net
    game = _game_of(C4)
    torch.manual_seed(0)
    net = Net(game.obs_shape, game.action_space).to(DEV).eval()
    for stagger in (True, False):
        buf = train.DeviceReplayBuffer(game, 100000, DEV)
        out = train.self_play(game, buf, net, 64, device=DEV, seed=4, searches=10, batch=8, stagger=stagger,
                              reuse=False, playout_cap=(0.3, 2))
        n_full = round(out["cap_full_share"] * out["cap_plies"])
        assert out["cap_plies"] == out["rows"] == out["steps"] + 64
        assert len(buf) == n_full and 0 < n_full < out["cap_plies"]
        assert 0.15 < out["cap_full_share"] < 0.45
        plain = train.DeviceReplayBuffer(game, 100000, DEV)
        ref = train.self_play(game, plain, net, 64, device=DEV, seed=4, searches=10, batch=8, stagger=stagger,
                              reuse=False)
        assert "cap_full_share" not in ref and len(plain) == ref["rows"]
    train.release_engines()


def test_cli_playout_cap_options_log_the_shares(tmp_path, monkeypatch):
    """test 6b: python -m caro_ai_amd.train with --playout-cap-full / --playout-cap-fast runs and logs the shares"""
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
                "--playout-cap-full", "0.25", "--playout-cap-fast", "3"])
    got = {r[0]: r[1] for r in rows}
    assert {"cap_full_share", "cap_fast_share"} <= set(got)
    assert 0.0 < got["cap_full_share"] < 1.0 and abs(got["cap_full_share"] + got["cap_fast_share"] - 1.0) < 1e-12
    assert any(line.startswith("Playout cap: full plies") for line in lines)
