"""SessionPool on the GPU: many human-vs-bot games as held / live slots of one lock-step engine (include/caro_hip.h,
"session pool").  Exact against the oracle with the table net, the properties of a held slot, the refusals, and the
shipped weights."""
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
from caro_ai_amd.lib.session_pool import SessionPool
from caro_ai_amd.net_hip import HashNet
from tests.conftest import WEIGHTS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED, SALT = 77, 5
E_INVAL, E_STATE = -22, -71


def _caro(n, k):
    from caro_ai_amd.lib.game.caro import Caro
    return Caro(n, k)


def _oracle(game):
    from oracle.oracle import Oracle
    if isinstance(game, ConnectFour):
        return Oracle(Oracle.C4)
    kind = Oracle.CARO if type(game).__name__ == "Caro" else Oracle.MNK
    return Oracle(kind, game.n, game.k)


def _pool(game, batch, evict=False, node_cap=None, slots=8, searches=3):
    return SessionPool(game, None, slots=slots, device=DEV, searches=searches, batch=batch, seed=SEED,
                       evaluator=HashNet(game, device=DEV, salt=SALT), evict=evict, node_cap=node_cap)


# ------------------------------------------------------------------ exact, against the oracle
GEOMETRIES = [
    ("c4-b8-k_tree", lambda: ConnectFour(), 8, False, None),
    ("c4-b4-dense", lambda: ConnectFour(), 4, False, None),
    ("ttt3-b8-k_tree_mw", lambda: TicTacToe(3, 3), 8, False, None),
    ("caro15-b8-k_tree_mw-evict", lambda: _caro(15, 5), 8, True, 1024),
]
OPENS = {0: [True, False], 1: [False], 2: [True], 4: [False, True]}  # round -> sessions opened (True: the human moves first)
CLOSES = {3: [0, 1]}                                                  # round -> sessions closed mid-game
ROUNDS = 14


@pytest.mark.parametrize("name,make_game,batch,evict,node_cap", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_six_sessions_play_their_oracle_games(name, make_game, batch, evict, node_cap):
    """Six sessions on a pool of eight slots, opened at different times, moved in changing subsets, two closed
    mid-game and their slots re-opened: at every bot turn the move, the value and (without eviction) the searched root's
    N / W / Q rows are those of an oracle that plays this session alone on its own kept store with the noise key
    (seed, uid, ply = moves so far, sim)."""
    game = make_game()
    S = 3
    pool = _pool(game, batch, evict=evict, node_cap=node_cap, searches=S)
    eng = pool.engine
    assert bool(eng.cfg.evict) == evict and eng.G == 8
    rng = random.Random(20261019)
    sessions, twins = [], []
    bot_turns = []  # per session
    subsets = set()
    for rnd in range(ROUNDS):
        for i in CLOSES.get(rnd, []):
            pool.close(sessions[i])
        for first in OPENS.get(rnd, []):
            s = pool.open(first, uid=7 * len(sessions) + 3)
            o = _oracle(game)
            o.use_synth_net(SALT)
            o.set_stream(SEED, s.uid)
            sessions.append(s)
            twins.append(o)
            bot_turns.append(0)
        if rnd == 4:  # sessions five and six sit in the slots of the two that were closed
            assert sorted((sessions[4].slot, sessions[5].slot)) == sorted((sessions[0].slot, sessions[1].slot))
        for s in sessions:
            if not s.closed and not s.finished and s.to_move == s.USER_PLAYER:
                move = rng.choice(game.possible_moves(s.state))
                before = s.state
                won = s.move_player(move)
                assert (s.state, won) == game.move(before, move, s.USER_PLAYER)
        ready = [s for s in sessions if s.bots_turn()]
        pick = ready if rnd % 3 == 0 else ready[:1] if rnd % 3 == 1 else ready[::-2]
        if not pick:
            continue
        subsets.add(len(pick))
        before = [(s.state, len(s.moves)) for s in pick]
        out = pool.move_bots(pick)
        for s, (state, ply), (move, value, won) in zip(pick, before, out):
            o = twins[sessions.index(s)]
            o.search_batch(S, batch, state, s.BOT_PLAYER, ply=ply)
            ref = o.get_node(state)
            want = int(np.argmax(o.get_policy(state, tau=0)))
            assert move == want, (name, rnd, s.uid, ply)
            assert value == ref["Q"][move], (name, rnd, s.uid, ply, value, ref["Q"][move])
            assert s.value == value and s.moves[-1] == move
            nxt, won_host = game.move(state, move, s.BOT_PLAYER)
            assert (s.state, won) == (nxt, won_host)
            assert s.is_draw() == (not game.possible_moves(nxt))
            if not evict:  # (with eviction the old root left the tree with the ply)
                nd = eng.lookup([s.slot], [0], [state])
                assert nd["found"][0] == 1
                assert nd["N"][0].tolist() == ref["N"].tolist(), (name, rnd, s.uid, ply)
                assert nd["W"][0].astype(np.float64).tolist() == ref["W"].tolist(), (name, rnd, s.uid, ply)
                assert nd["strong"][0].tolist() == ref["W_is_f32"].tolist()
                for a in range(game.action_space):
                    if ref["W_is_f32"][a]:
                        assert float(nd["Q"][0][a]) == ref["Q"][a]
                    else:
                        assert np.float32(ref["Q"][a]) == nd["Q"][0][a]
                assert int(eng.tree_sizes()[s.slot][0]) == o.store_len(0)
            bot_turns[sessions.index(s)] += 1
    # every session searched at least once, the two closed ones before they were closed; subsets of several sizes
    assert len(sessions) == 6 and min(bot_turns) >= 1 and len(subsets) >= 2, (bot_turns, subsets)
    assert eng.counters()["overflows"] == 0 and eng.pending_leaves() == 0
    pool.close_pool()


# ------------------------------------------------------------------ properties
def test_held_slots_are_untouched_by_a_move_of_the_others():
    game = ConnectFour()
    S, B = 3, 8
    pool = _pool(game, B, searches=S)
    eng = pool.engine
    rng = random.Random(3)
    sessions = [pool.open(i % 2 == 0) for i in range(6)]
    for _ in range(2):  # every session a few plies deep, each with a tree of its own
        for s in sessions:
            if s.to_move == s.USER_PLAYER:
                s.move_player(rng.choice(game.possible_moves(s.state)))
        pool.move_bots([s for s in sessions if s.bots_turn()])
    for s in sessions:
        if s.to_move == s.USER_PLAYER:
            s.move_player(rng.choice(game.possible_moves(s.state)))
    assert all(s.bots_turn() for s in sessions)
    assert eng.live_games() == 0
    subset = [sessions[1], sessions[4]]
    others = [g for g in range(eng.G) if g not in (subset[0].slot, subset[1].slot)]
    keys0, pl0, ply0, uid0 = eng.roots()
    sizes0, live0 = eng.tree_sizes(), eng.tree_live()
    c0 = eng.counters()
    pool.move_bots(subset)
    keys1, pl1, ply1, uid1 = eng.roots()
    sizes1, live1 = eng.tree_sizes(), eng.tree_live()
    c1 = eng.counters()
    for a, b in ((keys0, keys1), (pl0, pl1), (ply0, ply1), (uid0, uid1), (sizes0, sizes1), (live0, live1)):
        assert np.array_equal(a[others], b[others])
    for s in subset:
        assert ply1[s.slot] == ply0[s.slot] + 1 and pl1[s.slot] == s.USER_PLAYER
        assert game.from_key(keys1[s.slot]) == s.state
    assert c1["sims"] - c0["sims"] == S * B * len(subset)
    assert c1["plies"] - c0["plies"] == len(subset)
    assert eng.pending_leaves() == 0 and eng.live_games() == 0 and c1["overflows"] == 0
    pool.close_pool()


def _rc_of_pool_calls(eng, slot, hold=True):
    """the four calls (three without caro_pool_hold) with well-formed lists naming `slot`: their return codes"""
    L, st = eng.L, eng._stream()
    g = torch.tensor([slot], dtype=torch.int32, device=DEV)
    uid = torch.tensor([5], dtype=torch.int64, device=DEV)
    one = torch.tensor([1], dtype=torch.int32, device=DEV)
    keys = torch.from_numpy(eng.game.to_keys([eng.game.initial_state]).view(np.int64)).to(DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    rcs = (L.caro_pool_open(eng.h, 1, p(g), p(uid), p(one), st),
           L.caro_pool_set(eng.h, 1, p(g), p(keys), p(one), p(one), st),
           L.caro_pool_select(eng.h, 1, p(g), st))
    if hold:
        rcs += (L.caro_pool_hold(eng.h, st),)
    torch.cuda.synchronize()
    return rcs


def test_the_pool_calls_refuse_what_they_must():
    game = ConnectFour()
    S, B = 3, 8
    stag = SelfPlayEngine(game, 8, evaluators=[HashNet(game, device=DEV, salt=SALT)], max_batch=B, seed=SEED,
                          device=DEV, searches_hint=S, stagger=True)
    assert _rc_of_pool_calls(stag, 0) == (E_STATE,) * 4
    stag.search(S, B)  # the staggered engine goes on working
    assert stag.counters()["sims"] > 0 and stag.counters()["overflows"] == 0
    stag.close()

    eng = SelfPlayEngine(game, 8, evaluators=[HashNet(game, device=DEV, salt=SALT)], max_batch=B, seed=SEED,
                         steps_before_tau_0=0, device=DEV, searches_hint=S)
    for bad in (8, -1, 1 << 20):
        assert _rc_of_pool_calls(eng, bad, hold=False) == (E_INVAL,) * 3, bad
    L, st = eng.L, eng._stream()
    two = torch.tensor([2, 2], dtype=torch.int32, device=DEV)
    assert L.caro_pool_select(eng.h, 2, C.c_void_p(two.data_ptr()), st) == E_INVAL  # a slot named twice
    assert L.caro_pool_select(eng.h, -1, C.c_void_p(two.data_ptr()), st) == E_INVAL
    assert L.caro_pool_select(eng.h, 1, None, st) == E_INVAL
    g = torch.tensor([1], dtype=torch.int32, device=DEV)
    keys = torch.from_numpy(game.to_keys([game.initial_state]).view(np.int64)).to(DEV)
    one = torch.tensor([1], dtype=torch.int32, device=DEV)
    far = torch.tensor([42], dtype=torch.int32, device=DEV)  # a ply the history has no row for
    assert L.caro_pool_set(eng.h, 1, C.c_void_p(g.data_ptr()), C.c_void_p(keys.data_ptr()), C.c_void_p(one.data_ptr()),
                           C.c_void_p(far.data_ptr()), st) == E_INVAL
    with pytest.raises(_lib.CaroError):
        eng.pool_select([8])
    # nothing was changed by the refusals: all eight games are live and the engine plays on
    assert eng.live_games() == 8
    eng.search(S, B)
    eng.step()
    c = eng.counters()
    assert c["sims"] == 8 * S * B and c["plies"] == 8 and c["overflows"] == 0
    # and the calls work on it: hold everything, let two slots search
    eng.pool_hold()
    assert eng.live_games() == 0
    eng.pool_select([6, 1])
    assert eng.live_games() == 2
    eng.search(S, B)
    eng.pool_hold()
    assert eng.counters()["sims"] == 10 * S * B and eng.live_games() == 0
    eng.close()


# ------------------------------------------------------------------ the shipped weights
@pytest.fixture(scope="module")
def c4_pool():
    pool = SessionPool(ConnectFour(), os.path.join(WEIGHTS, "best_026_12000.dat"), slots=8, device=DEV, seed=SEED)
    yield pool
    pool.close_pool()


def test_four_sessions_with_the_shipped_weights_run_to_the_end(c4_pool):
    pool, game = c4_pool, c4_pool.game
    assert (pool.searches, pool.batch) == (40, 8) and type(pool.evaluator).__name__ == "HipNet"
    rng = random.Random(11)
    sessions = [pool.open(i % 2 == 0) for i in range(4)]
    for _ in range(43):
        for s in sessions:
            if not s.finished and s.to_move == s.USER_PLAYER:
                s.move_player(rng.choice(game.possible_moves(s.state)))
        ready = [s for s in sessions if s.bots_turn()]
        if not ready:
            break
        for (move, value, won), s in zip(pool.move_bots(ready), ready):
            assert np.isfinite(value) and -1.0 <= float(value) <= 1.0
            assert s.moves[-1] == move and s.finished == (won or s.is_draw())
    assert all(s.finished for s in sessions)
    assert pool.engine.counters()["overflows"] == 0
    for s in sessions:
        pool.close(s)


def test_the_bot_takes_a_win_in_one(c4_pool):
    pool, game = c4_pool, c4_pool.game
    s = pool.open(False)
    bot, user = s.BOT_PLAYER, s.USER_PLAYER
    state, moves = game.initial_state, []
    for who, col in ((bot, 0), (user, 6), (bot, 1), (user, 6), (bot, 2), (user, 5)):  # the bot: three in the bottom row
        state, won = game.move(state, col, who)
        moves.append(col)
        assert not won
    assert game.move(state, 3, bot)[1]
    s.state, s.moves, s.to_move = state, moves, bot
    pool.engine.pool_set([s.slot], [state], [bot], [len(moves)])
    (move, value, won), = pool.move_bots([s])
    assert move == 3 and won and s.finished
    assert np.isfinite(value) and -1.0 <= float(value) <= 1.0
    pool.close(s)
