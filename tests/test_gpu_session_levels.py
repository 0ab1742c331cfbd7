"""Session levels on the GPU (include/caro_hip.h, "session pool": LEVELS): sessions of one pool with their own minibatch
budget, move temperature and net, searched in the same launches.  Exact against the oracle with two table nets, levels
that say nothing, independence of the neighbours, caro_search_move, the refusals, and the shipped weights."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

from caro_ai_amd import _lib
from caro_ai_amd.engine import SelfPlayEngine
from caro_ai_amd.lib.game.connect_four import ConnectFour
from caro_ai_amd.lib.game.tictactoe import TicTacToe
from caro_ai_amd.lib.session_pool import Level, SessionPool
from caro_ai_amd.net_hip import HashNet
from oracle.oracle import sample_index
from tests.conftest import WEIGHTS
from tests.test_gpu_session_pool import GEOMETRIES, _oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED, SALT0, SALT1 = 77, 5, 11
E_INVAL, E_STATE = -22, -71


def _nets(game):
    return [HashNet(game, device=DEV, salt=SALT0), HashNet(game, device=DEV, salt=SALT1)]


def _pool(game, batch, evict=False, node_cap=None, slots=8, searches=3, two=True):
    ev = _nets(game) if two else HashNet(game, device=DEV, salt=SALT0)
    return SessionPool(game, None, slots=slots, device=DEV, searches=searches, batch=batch, seed=SEED, evaluator=ev,
                       evict=evict, node_cap=node_cap)


def _twin(game, uid):
    o = _oracle(game)
    o.use_synth_net(SALT0, SALT1)
    o.set_stream(SEED, uid)
    return o


def _twin_move(game, N, tau, uid, ply):
    """sample_index(caro_host_temperature(N, tau), caro_host_move_uniform(seed, uid, ply))"""
    L = _lib.load()
    n = np.ascontiguousarray(N, dtype=np.int32)
    pi = np.zeros(game.action_space)
    assert L.caro_host_temperature(game.action_space, n.ctypes.data, float(tau), pi.ctypes.data) >= 0
    return sample_index(pi, L.caro_host_move_uniform(SEED, int(uid), int(ply)))


def _assert_root_is(eng, game, slot, state, ref, where):
    nd = eng.lookup([slot], [0], [state])
    assert nd["found"][0] == 1, where
    assert nd["N"][0].tolist() == ref["N"].tolist(), where
    assert nd["W"][0].astype(np.float64).tolist() == ref["W"].tolist(), where
    assert nd["strong"][0].tolist() == ref["W_is_f32"].tolist(), where
    for a in range(game.action_space):
        if ref["W_is_f32"][a]:
            assert float(nd["Q"][0][a]) == ref["Q"][a], where
        else:
            assert np.float32(ref["Q"][a]) == nd["Q"][0][a], where


# ------------------------------------------------------------------ 1: exact, against the oracle
# searches from {2, 3, 5}, tau from {0, 1, 0.5}, net from {0, 1}; None: the pool's own (3 minibatches, tau 0, net 0)
LEVELS = [Level(2, 0.0, 0), Level(3, 1.0, 1), Level(5, 0.5, 0), Level(2, 0.5, 1), None, Level(5, 0.0, 1)]
OPENS = {0: [True, False], 1: [False], 2: [True], 4: [False, True]}  # round -> sessions opened (True: the human moves first)
CLOSES = {3: [0]}             # session 0 leaves; session 4 (no level) takes its slot, which must be back at (net 0, tau 0)
RELEVEL = {3: (2, Level(3, 1.0, 1))}  # round -> (session, its new level): budget, temperature and net change mid-game
ROUNDS = 14


@pytest.mark.parametrize("name,make_game,batch,evict,node_cap", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_six_sessions_of_different_levels_play_their_oracle_games(name, make_game, batch, evict, node_cap):
    """At every bot turn the move is the one the session's level samples from its oracle twin's root -- searched alone,
    level.searches minibatches with the level's net -- the value is the twin's Q[move], and (without eviction) the
    searched root's rows and the tree size are the twin's.  Every call counts batch x (the sum of the budgets) sims."""
    game = make_game()
    S = 3
    pool = _pool(game, batch, evict=evict, node_cap=node_cap, searches=S)
    eng = pool.engine
    assert bool(eng.cfg.evict) == evict and eng.G == 8 and eng.n_nets == 2 and eng.n_stores == 1
    rng = random.Random(20261020)
    sessions, twins, bot_turns = [], [], []
    mixed_calls, nets_used, taus_used, releveled = 0, set(), set(), None
    for rnd in range(ROUNDS):
        for i in CLOSES.get(rnd, []):
            pool.close(sessions[i])
        for first in OPENS.get(rnd, []):
            s = pool.open(first, uid=7 * len(sessions) + 3, level=LEVELS[len(sessions)])
            sessions.append(s)
            twins.append(_twin(game, s.uid))
            bot_turns.append(0)
        if rnd == 4:
            assert sessions[4].slot == sessions[0].slot and sessions[4].level is None
        if rnd in RELEVEL:
            i, level = RELEVEL[rnd]
            assert not sessions[i].finished and sessions[i].level != level
            sessions[i].set_level(level)
            releveled = bot_turns[i]
        for s in sessions:
            if not s.closed and not s.finished and s.to_move == s.USER_PLAYER:
                s.move_player(rng.choice(game.possible_moves(s.state)))
        ready = [s for s in sessions if s.bots_turn()]
        pick = ready if rnd % 3 == 0 else ready[:1] if rnd % 3 == 1 else ready[::-2]
        if not pick:
            continue
        levels = [s.level or Level(S, 0.0, 0) for s in pick]
        budgets = [lv.searches for lv in levels]
        mixed_calls += len(set(budgets)) > 1
        before = [(s.state, len(s.moves)) for s in pick]
        sims0 = eng.counters()["sims"]
        out = pool.move_bots(pick)
        assert eng.counters()["sims"] - sims0 == batch * sum(budgets), (name, rnd, budgets)
        for s, lv, (state, ply), (move, value, won) in zip(pick, levels, before, out):
            where = (name, rnd, s.uid, ply, lv)
            o = twins[sessions.index(s)]
            o.search_batch(lv.searches, batch, state, s.BOT_PLAYER, which_net=lv.net, ply=ply)
            ref = o.get_node(state)
            assert move == _twin_move(game, ref["N"], lv.tau, s.uid, ply), where
            assert value == ref["Q"][move], where + (value, ref["Q"][move])
            assert s.value == value and s.moves[-1] == move
            nxt, won_host = game.move(state, move, s.BOT_PLAYER)
            assert (s.state, won) == (nxt, won_host)
            if not evict:  # (with eviction the old root left the tree with the ply)
                _assert_root_is(eng, game, s.slot, state, ref, where)
                assert int(eng.tree_sizes()[s.slot][0]) == o.store_len(0), where
            bot_turns[sessions.index(s)] += 1
            nets_used.add(lv.net)
            taus_used.add(lv.tau)
    assert len(sessions) == 6 and min(bot_turns) >= 1 and bot_turns[RELEVEL[3][0]] > releveled, bot_turns
    assert mixed_calls >= 1 and nets_used == {0, 1} and taus_used == {0.0, 0.5, 1.0}, (mixed_calls, nets_used, taus_used)
    assert eng.counters()["overflows"] == 0 and eng.pending_leaves() == 0
    pool.close_pool()


# ------------------------------------------------------------------ 2 and 3: one scripted run, several pools
def _run(game, batch, levels, searches=3, two=False, rounds=6, watch=None):
    """Four sessions (uids 3, 10, 17, 24; the even ones human-first) with the given levels (None: open() without one)
    against one scripted human; returns, per session, [(move, value, N, W, Q, strong of the searched root)] -- of the
    sessions in `watch` only, if given -- and the engine's kernel form."""
    pool = _pool(game, batch, searches=searches, two=two, slots=4)
    eng = pool.engine
    sessions = [pool.open(i % 2 == 0, uid=7 * i + 3, **({} if lv is None else {"level": lv})) for i, lv in enumerate(levels)]
    log = [[] for _ in sessions]
    for rnd in range(rounds):
        for s in sessions:
            if not s.finished and s.to_move == s.USER_PLAYER:
                moves = sorted(game.possible_moves(s.state))
                s.move_player(moves[(3 * rnd + s.uid) % len(moves)])
        ready = [s for s in sessions if s.bots_turn()]
        if rnd % 2:
            ready = ready[::-1]
        if not ready:
            break
        before = [s.state for s in ready]
        for s, state, (move, value, _) in zip(ready, before, pool.move_bots(ready)):
            nd = eng.lookup([s.slot], [0], [state])
            assert nd["found"][0] == 1
            log[sessions.index(s)].append((move, float(value)) + tuple(nd[k][0].tolist() for k in ("N", "W", "Q", "strong")))
    assert eng.counters()["overflows"] == 0
    lean = eng.L.caro_engine_kernel_form(eng.h) == 0
    pool.close_pool()
    return ([log[i] for i in watch] if watch is not None else log), lean


@pytest.mark.parametrize("make_game,batch", [(lambda: ConnectFour(), 8), (lambda: TicTacToe(3, 3), 8)], ids=["c4-b8", "ttt3-b8"])
def test_levels_that_say_nothing_change_nothing(make_game, batch):
    game = make_game()
    plain, lean = _run(game, batch, [None] * 4)
    said, lean_said = _run(game, batch, [Level(3, 0.0, 0)] * 4)
    assert lean and not lean_said  # the pool without levels never told its engine of them; the other runs the full form
    assert all(len(x) >= 2 for x in plain)
    assert said == plain


def test_a_session_does_not_depend_on_the_levels_beside_it():
    game = ConnectFour()
    mine = Level(3, 0.5, 1)
    a, _ = _run(game, 8, [Level(5, 1.0, 0), mine, Level(2, 0.0, 1), None], two=True, watch=[1])
    b, _ = _run(game, 8, [Level(2, 0.5, 1), mine, Level(5, 1.0, 0), Level(5, 0.0, 1)], two=True, watch=[1])
    c, _ = _run(game, 8, [None, mine, None, None], two=True, watch=[1])
    assert len(a[0]) >= 3 and a == b == c


# ------------------------------------------------------------------ 4: caro_search_move
def test_search_move_with_budgets_and_temperatures_is_search_then_step():
    """3 x 3 at batch 8: the ply rides in k_tree_mw's closing launch"""
    game = TicTacToe(3, 3)
    S, B, G = 5, 8, 8
    slots, budgets = [6, 1, 3, 4], [2, 5, 3, 9]  # (9: above the call's searches = the call's searches)
    nets, taus = [1, 0, 1, 0], [1.0, 0.5, 0.0, 2.0]
    got = []
    for one_call in (False, True):
        eng = SelfPlayEngine(game, G, evaluators=_nets(game), n_stores=1, max_batch=B, seed=SEED, steps_before_tau_0=0,
                             first_player_mode=0, device=DEV, searches_hint=S)
        eng.pool_level([], [], [])
        eng.pool_hold()
        eng.pool_open(slots, [40 + g for g in slots], [0, 1, 0, 1])
        eng.pool_level(slots, nets, taus)
        plies = []
        for _ in range(3):
            eng.pool_select_budget(slots, budgets)
            sims0 = eng.counters()["sims"]
            actions = torch.full((G,), -7, dtype=torch.int32, device=DEV)
            done = torch.full((G,), -7, dtype=torch.int32, device=DEV)
            result = torch.full((G,), -7, dtype=torch.int32, device=DEV)
            if one_call:
                p = lambda t: C.c_void_p(t.data_ptr())
                _lib.check(eng.L.caro_search_move(eng.h, eng.evaluators[0].h, eng.evaluators[1].h, S, B, None, None,
                                                  p(eng.planes), p(eng.leaf_keys), p(eng._probs), p(eng._values),
                                                  p(actions), p(done), p(result), eng._stream()))
            else:
                eng.search(S, B)
                actions, done, result = eng.step()
            eng.pool_hold()
            keys, pl, ply, uid = eng.roots()
            live = [g for g, b in zip(slots, budgets) if ply[g] > len(plies)]  # slots that made this ply
            assert eng.counters()["sims"] - sims0 == B * sum(min(b, S) for g, b in zip(slots, budgets) if g in live)
            plies.append((actions.cpu().tolist(), done.cpu().tolist(), keys.tolist(), pl.tolist(), ply.tolist()))
        c = eng.counters()
        assert c["overflows"] == 0 and c["plies"] >= 8
        got.append(plies)
        eng.close()
    assert got[0] == got[1]
    first_actions = got[0][0][0]
    assert all(first_actions[g] >= 0 for g in slots) and all(first_actions[g] == -1 for g in range(G) if g not in slots)


# ------------------------------------------------------------------ 5: refusals
def _p(t):
    return C.c_void_p(t.data_ptr())


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def _f64(x):
    return torch.tensor(x, dtype=torch.float64, device=DEV)


def _level_rc(eng, slots, nets, taus):
    g, n, t = _i32(slots), _i32(nets), _f64(taus)  # (held until the call has returned)
    rc = eng.L.caro_pool_level(eng.h, len(slots), _p(g), _p(n), _p(t), eng._stream())
    torch.cuda.synchronize()
    return rc


def _budget_rc(eng, slots, budgets):
    g, b = _i32(slots), _i32(budgets)
    rc = eng.L.caro_pool_select_budget(eng.h, len(slots), _p(g), _p(b), eng._stream())
    torch.cuda.synchronize()
    return rc


def test_the_level_calls_refuse_what_they_must():
    game = ConnectFour()
    S, B = 3, 8
    mk = lambda nets, **kw: SelfPlayEngine(game, 8, evaluators=nets, max_batch=B, seed=SEED, device=DEV, searches_hint=S,
                                           **kw)
    # a staggered engine
    stag = mk(_nets(game)[:1], stagger=True)
    assert _level_rc(stag, [0], [0], [0.0]) == E_STATE and _budget_rc(stag, [0], [2]) == E_STATE
    stag.search(S, B)
    assert stag.counters()["sims"] > 0 and stag.counters()["overflows"] == 0
    stag.close()
    # an engine with the playout cap set; and the cap's setter once levels are on
    cap = mk(_nets(game)[:1], steps_before_tau_0=0)
    cap.set_playout_cap(0.5, 2)
    assert _level_rc(cap, [0], [0], [0.0]) == E_STATE and _budget_rc(cap, [0], [2]) == E_STATE
    assert cap.L.caro_engine_kernel_form(cap.h) == 1  # (the cap's doing; levels did not come on)
    cap.search(S, B)
    cap.step()
    assert cap.counters()["plies"] == 8 and cap.counters()["overflows"] == 0
    cap.close()

    eng = mk(_nets(game), steps_before_tau_0=0, n_stores=1)
    L, st = eng.L, eng._stream()
    # the plain pool calls on two nets, before levels are on: every refusal of today stays
    g, one = _i32([1]), _i32([1])
    uid = torch.tensor([5], dtype=torch.int64, device=DEV)
    keys = torch.from_numpy(game.to_keys([game.initial_state]).view(np.int64)).to(DEV)
    assert (L.caro_pool_open(eng.h, 1, _p(g), _p(uid), _p(one), st), L.caro_pool_set(eng.h, 1, _p(g), _p(keys), _p(one), _p(one), st),
            L.caro_pool_select(eng.h, 1, _p(g), st), L.caro_pool_hold(eng.h, st)) == (E_STATE,) * 4
    assert eng.L.caro_engine_kernel_form(eng.h) == 0
    # bad lists: the code, and levels stay off (the engine keeps its lean kernels, the plain calls stay refused)
    assert _level_rc(eng, [1], [2], [0.0]) == E_INVAL      # net out of range
    assert _level_rc(eng, [1], [-1], [0.0]) == E_INVAL
    assert _level_rc(eng, [1], [0], [0.01]) == E_INVAL     # tau below 0.05
    assert _level_rc(eng, [1], [0], [9.0]) == E_INVAL      # tau above 8
    assert _level_rc(eng, [2, 2], [0, 1], [0.0, 0.0]) == E_INVAL  # a slot named twice
    assert _level_rc(eng, [8], [0], [0.0]) == E_INVAL
    assert _budget_rc(eng, [1], [0]) == E_INVAL            # budget 0
    assert _budget_rc(eng, [1, 2], [3, -2]) == E_INVAL
    assert _budget_rc(eng, [3, 3], [2, 2]) == E_INVAL
    zero = _f64([0.0])
    assert L.caro_pool_level(eng.h, 1, _p(g), None, _p(zero), st) == E_INVAL
    assert L.caro_pool_select_budget(eng.h, 1, _p(g), None, st) == E_INVAL
    assert eng.L.caro_engine_kernel_form(eng.h) == 0 and L.caro_pool_hold(eng.h, st) == E_STATE
    # nothing was changed: all eight games are live and play on, each mover with its own net
    assert eng.live_games() == 8
    eng.search(S, B)
    eng.step()
    c = eng.counters()
    assert c["sims"] == 8 * S * B and c["plies"] == 8 and c["overflows"] == 0
    # levels on: the refused values are still refused and leave the slot's level alone; the three setters are refused
    eng.pool_level([], [], [])
    assert eng.L.caro_engine_kernel_form(eng.h) == 1
    eng.pool_hold()
    eng.pool_open([1, 6], [21, 22], [0, 0])
    eng.pool_level([1], [1], [0.5])
    assert _level_rc(eng, [1], [2], [0.0]) == E_INVAL and _level_rc(eng, [1], [0], [9.0]) == E_INVAL
    assert _budget_rc(eng, [1, 6], [2, 0]) == E_INVAL and eng.live_games() == 0
    assert L.caro_engine_set_playout_cap(eng.h, C.c_double(0.5), 2) == E_STATE
    assert L.caro_engine_set_early_stop(eng.h, 1) == E_STATE
    assert L.caro_engine_set_temperature(eng.h, C.c_double(0.5), C.c_double(0.5), 0) == E_STATE
    with pytest.raises(_lib.CaroError):
        eng.pool_select_budget([1], [0])
    # the engine plays on: slot 1 at (net 1, tau 0.5, 2 minibatches), slot 6 at (net 0, tau 0, all 3)
    s0 = eng.counters()["sims"]
    eng.pool_select_budget([6, 1], [3, 2])
    assert eng.live_games() == 2
    eng.search(S, B)
    rows = eng.lookup([1, 6], [0, 0], [game.initial_state] * 2)
    actions, done, _ = eng.step()
    eng.pool_hold()
    assert eng.counters()["sims"] - s0 == 5 * B and eng.live_games() == 0 and eng.counters()["overflows"] == 0
    for i, (slot, uid_, net, tau, b) in enumerate(((1, 21, 1, 0.5, 2), (6, 22, 0, 0.0, 3))):
        o = _twin(game, uid_)
        o.search_batch(b, B, game.initial_state, 0, which_net=net, ply=0)
        ref = o.get_node(game.initial_state)
        assert rows["N"][i].tolist() == ref["N"].tolist()
        assert int(actions[slot]) == _twin_move(game, ref["N"], tau, uid_, 0)
    eng.close()


# ------------------------------------------------------------------ 6: the shipped weights
def test_four_levels_with_two_shipped_nets_run_to_the_end():
    files = [os.path.join(WEIGHTS, "best_026_12000.dat"), os.path.join(WEIGHTS, "best_025_10600.dat")]
    pool = SessionPool(ConnectFour(), files, slots=8, device=DEV, seed=SEED)
    game = pool.game
    assert pool.model_files == files and pool.model_file == files[0] and len(pool.models) == 2
    assert pool.model is pool.models[0] and pool.engine.n_nets == 2 and (pool.searches, pool.batch) == (40, 8)
    rng = random.Random(11)
    levels = [None, Level(10, 1.0, 1), Level(20, 0.5, 0), Level(2, 0.0, 1)]
    sessions = [pool.open(i % 2 == 0, level=lv) for i, lv in enumerate(levels)]
    for _ in range(43):
        for s in sessions:
            if not s.finished and s.to_move == s.USER_PLAYER:
                s.move_player(rng.choice(game.possible_moves(s.state)))
        ready = [s for s in sessions if s.bots_turn()]
        if not ready:
            break
        sims0 = pool.engine.counters()["sims"]
        out = pool.move_bots(ready)  # (raises if a slot and the host disagree about the end of a game)
        assert pool.engine.counters()["sims"] - sims0 == 8 * sum((s.level or Level(40)).searches or 40 for s in ready)
        for (move, value, won), s in zip(out, ready):
            assert np.isfinite(value) and -1.0 <= float(value) <= 1.0
            assert s.moves[-1] == move and s.finished == (won or s.is_draw())
    assert all(s.finished for s in sessions)
    assert pool.engine.counters()["overflows"] == 0
    pool.close_pool()
