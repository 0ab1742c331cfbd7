"""SessionPool without a GPU: the four C symbols, PooledSession against Session's public names, and the pool's
bookkeeping against a stub engine that records the calls it gets."""
import ctypes as C

import pytest
import torch

from caro_ai_amd import _lib
from caro_ai_amd.lib.game.connect_four import ConnectFour
from caro_ai_amd.lib.play_session import Session
from caro_ai_amd.lib.session_pool import PooledSession, SessionPool

E_INVAL = -22
POOL_SYMBOLS = ("caro_pool_open", "caro_pool_set", "caro_pool_select", "caro_pool_hold")


def test_the_four_symbols_are_exported_and_refuse_null_arguments():
    L = _lib.load()
    for name in POOL_SYMBOLS:
        assert hasattr(L, name) and name in _lib.EXPORTS
    assert L.caro_version() == 107
    lst = (C.c_int32 * 1)(0)  # (a host list: never read, the handle is refused first)
    p = C.cast(lst, C.c_void_p)
    assert L.caro_pool_open(None, 1, p, p, p, None) == E_INVAL
    assert L.caro_pool_set(None, 1, p, p, p, p, None) == E_INVAL
    assert L.caro_pool_select(None, 1, p, None) == E_INVAL
    assert L.caro_pool_hold(None, None) == E_INVAL
    assert L.caro_pool_open(None, 0, None, None, None, None) == E_INVAL
    assert L.caro_pool_set(None, 0, None, None, None, None, None) == E_INVAL
    assert L.caro_pool_select(None, 0, None, None) == E_INVAL
    assert b"null" in L.caro_last_error()


class StubEngine:
    """what SessionPool asks of a SelfPlayEngine; plays every listed slot's lowest legal move"""

    def __init__(self, game, n):
        self.game, self.G = game, n
        self.calls = []
        self.overflows = 0
        self._looked = None

        class Cfg:
            node_cap = 0
        self.cfg = Cfg()

    def pool_open(self, slots, uids, first_players):
        self.calls.append(("pool_open", list(slots), list(uids), list(first_players)))

    def pool_set(self, slots, states, players, plies):
        self.calls.append(("pool_set", list(slots), list(states), list(players), list(plies)))

    def pool_select(self, slots):
        self.calls.append(("pool_select", list(slots)))

    def search(self, searches, batch):
        self.calls.append(("search", searches, batch))

    def lookup_dev(self, games, stores, states):
        self.calls.append(("lookup_dev", list(games)))
        self._looked = (list(games), list(states))
        M, A = len(states), self.game.action_space
        rows = {"found": torch.ones(M, dtype=torch.int32), "N": torch.ones((M, A), dtype=torch.int32),
                "strong": torch.zeros((M, A), dtype=torch.int32)}
        for k in ("W", "Q", "P"):
            rows[k] = torch.full((M, A), 0.5)
        return rows

    def step(self):
        self.calls.append(("step",))
        actions = torch.full((self.G,), -1, dtype=torch.int32)
        done = torch.ones(self.G, dtype=torch.int32)
        for g, state in zip(*self._looked):
            move = min(self.game.possible_moves(state))
            nxt, won = self.game.move(state, move, self.game.player_black)
            actions[g] = move
            done[g] = int(won or not self.game.possible_moves(nxt))
        return actions, done, torch.zeros(self.G, dtype=torch.int32)

    def pool_hold(self):
        self.calls.append(("pool_hold",))

    def counters(self):
        self.calls.append(("counters",))
        return {"overflows": self.overflows}


def _pool(slots=4):
    game = ConnectFour()
    eng = StubEngine(game, slots)
    return SessionPool(game, "weights.dat", slots=slots, device="cpu", searches=5, batch=8, engine=eng), eng


def test_pooled_session_has_every_public_name_of_session():
    pool, _ = _pool()
    s = pool.open(True)
    have = set(dir(s))
    for name in dir(Session):
        if not name.startswith("_"):
            assert name in have, name
    # and the attributes Session.__init__ sets (lib/play_session.py:8-21)
    for name in ("game", "BOT_PLAYER", "USER_PLAYER", "model_file", "model", "state", "value", "player_moves_first",
                 "moves", "mcts_store"):
        assert name in have, name
    assert isinstance(s, PooledSession)
    assert (s.BOT_PLAYER, s.USER_PLAYER) == (pool.game.player_black, pool.game.player_white)
    assert s.state == pool.game.initial_state and s.moves == [] and s.value is None
    assert s.render() == "<pre>%s</pre>" % pool.game.render(s.state)


def test_open_hands_out_the_lowest_free_slot_and_a_counter_uid():
    pool, eng = _pool(3)
    a, b = pool.open(True), pool.open(False)
    assert (a.slot, a.uid, b.slot, b.uid) == (0, 0, 1, 1)
    bot, user = a.BOT_PLAYER, a.USER_PLAYER
    assert eng.calls == [("pool_open", [0], [0], [user]), ("pool_open", [1], [1], [bot])]
    c = pool.open(True, uid=40)
    assert (c.slot, c.uid) == (2, 40)
    with pytest.raises(RuntimeError, match="pool is full"):
        pool.open(True)
    assert len(eng.calls) == 3  # the refused open reached no engine call
    pool.close(b)
    d = pool.open(False)
    assert (d.slot, d.uid) == (1, 41)  # the freed slot again, cleared by a pool_open of its own
    assert eng.calls[-1] == ("pool_open", [1], [41], [bot])
    with pytest.raises(ValueError):
        pool.close(b)


def test_move_player_pushes_the_new_root_and_checks_the_move():
    pool, eng = _pool()
    game = pool.game
    s = pool.open(True)
    del eng.calls[:]
    won = s.move_player(3)
    state, _ = game.move(game.initial_state, 3, s.USER_PLAYER)
    assert not won and s.state == state and s.moves == [3]
    assert eng.calls == [("pool_set", [s.slot], [state], [s.BOT_PLAYER], [1])]
    del eng.calls[:]
    with pytest.raises(ValueError):  # out of turn
        s.move_player(3)
    t = pool.open(True)
    del eng.calls[:]
    with pytest.raises(ValueError):  # not a column
        t.move_player(7)
    assert eng.calls == []


def test_move_bots_selects_exactly_the_listed_slots_then_searches_then_holds():
    pool, eng = _pool()
    game = pool.game
    a, b, c = pool.open(False), pool.open(True), pool.open(False)
    del eng.calls[:]
    out = pool.move_bots([c, a])
    assert [x[0] for x in eng.calls] == ["pool_select", "search", "lookup_dev", "step", "pool_hold", "counters"]
    assert eng.calls[0] == ("pool_select", [c.slot, a.slot]) and eng.calls[1] == ("search", 5, 8)
    assert eng.calls[2] == ("lookup_dev", [c.slot, a.slot])
    assert [o[0] for o in out] == [0, 0] and [o[2] for o in out] == [False, False]
    for s, (move, value, won) in zip((c, a), out):
        assert s.moves == [move] and s.value == value == 0.5 and s.to_move == s.USER_PLAYER
        assert s.state == game.move(game.initial_state, move, s.BOT_PLAYER)[0]
    assert b.moves == [] and b.state == game.initial_state
    del eng.calls[:]
    assert a.move_bot.__self__ is a
    a.move_player(1)
    assert a.move_bot() is False  # move_bot() is move_bots([self])
    assert ("pool_select", [a.slot]) in eng.calls


def test_move_bots_refuses_before_any_engine_call():
    pool, eng = _pool()
    other, _ = _pool()
    a, b = pool.open(False), pool.open(True)
    foreign = other.open(False)
    closed = pool.open(False)
    pool.close(closed)
    finished = pool.open(False)
    finished.finished = True
    del eng.calls[:]
    for bad in ([a, a], [b], [a, closed], [foreign], [finished], [a, object()]):
        with pytest.raises(ValueError):
            pool.move_bots(bad)
    assert eng.calls == [] and a.moves == []
    assert pool.move_bots([]) == [] and eng.calls == []
    eng.overflows = 1
    with pytest.raises(_lib.CaroError):  # an overflow is an error, as everywhere else
        pool.move_bots([a])
