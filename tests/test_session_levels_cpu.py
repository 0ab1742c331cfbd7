"""Session levels without a GPU: the two C symbols, `Level`'s checks, and the engine calls a pool with levels makes,
against the stub engine of tests/test_session_pool_cpu.py."""
import ctypes as C

import pytest

from caro_ai_amd import _lib
from caro_ai_amd.lib.game.connect_four import ConnectFour
from caro_ai_amd.lib.session_pool import Level, SessionPool
from tests.test_session_pool_cpu import StubEngine

E_INVAL = -22


class LevelStub(StubEngine):
    def pool_level(self, slots, nets, taus):
        self.calls.append(("pool_level", list(slots), list(nets), list(taus)))

    def pool_select_budget(self, slots, budgets):
        self.calls.append(("pool_select_budget", list(slots), list(budgets)))


def _pool(slots=4, files="weights.dat"):
    game = ConnectFour()
    eng = LevelStub(game, slots)
    return SessionPool(game, files, slots=slots, device="cpu", searches=5, batch=8, engine=eng), eng


def test_the_two_symbols_are_exported_and_refuse_null_arguments():
    L = _lib.load()
    for name in ("caro_pool_level", "caro_pool_select_budget"):
        assert hasattr(L, name) and name in _lib.EXPORTS
    assert L.caro_version() == 107
    lst = (C.c_int32 * 2)(0, 0)  # (a host list: never read, the handle is refused first)
    p = C.cast(lst, C.c_void_p)
    assert L.caro_pool_level(None, 1, p, p, p, None) == E_INVAL
    assert L.caro_pool_select_budget(None, 1, p, p, None) == E_INVAL
    assert L.caro_pool_level(None, 0, None, None, None, None) == E_INVAL
    assert L.caro_pool_select_budget(None, 0, None, None, None) == E_INVAL
    assert b"null" in L.caro_last_error()


def test_level_defaults_and_checks():
    assert Level() == (None, 0.0, 0)
    assert Level(3, 0.5, 1).checked() == Level(3, 0.5, 1)
    assert Level(2, 0, 0).checked() == Level(2, 0.0, 0) and isinstance(Level(2, 0, 0).checked().tau, float)
    assert Level(tau=0.05).checked().tau == 0.05 and Level(tau=8).checked().tau == 8.0
    for bad in (Level(1), Level(0), Level(-3), Level(2.5), Level(True), Level("3"),
                Level(tau=0.01), Level(tau=9), Level(tau=-1), Level(tau=float("nan")), Level(tau="warm"), Level(tau=None),
                Level(net=2), Level(net=-1), Level(net=0.0), Level(net=True), Level(net=None)):
        with pytest.raises(ValueError):
            bad.checked()
    with pytest.raises(ValueError):  # the pool has one net
        Level(net=1).checked(n_nets=1)


def test_a_pool_of_one_net_refuses_the_second_and_a_pool_takes_at_most_two():
    pool, eng = _pool()
    with pytest.raises(ValueError):
        pool.open(True, level=Level(net=1))
    assert eng.calls == [] and len(pool._free) == 4  # no slot was taken, no call went out
    with pytest.raises(ValueError):
        _pool(files=("a.dat", "b.dat", "c.dat"))
    two, _ = _pool(files=("a.dat", "b.dat"))
    assert two.model_files == ["a.dat", "b.dat"] and two.model_file == "a.dat" and two.n_nets == 2
    s = two.open(True, level=Level(net=1))
    assert s.level == Level(None, 0.0, 1) and s.model_file == "a.dat"


def test_a_pool_without_levels_makes_the_calls_it_always_made():
    pool, eng = _pool()
    a, b = pool.open(False), pool.open(False, level=None)
    a.set_level(None)  # nobody ever had a level: nothing to say
    assert a.level is None
    pool.move_bots([b, a])
    assert [c[0] for c in eng.calls] == ["pool_open", "pool_open", "pool_select", "search", "lookup_dev", "step",
                                         "pool_hold", "counters"]
    assert eng.calls[2] == ("pool_select", [b.slot, a.slot]) and eng.calls[3] == ("search", 5, 8)


def test_a_mixed_level_move_states_a_budget_per_slot_and_searches_the_largest():
    pool, eng = _pool(slots=5, files=("a.dat", "b.dat"))
    a = pool.open(False, level=Level(3, 0.5, 1))
    b = pool.open(False)                          # no level of its own: the pool's searches
    c = pool.open(False, level=Level(tau=1.0))    # searches=None: the pool's searches too
    d = pool.open(False, level=Level(2))
    assert eng.calls == [("pool_open", [0], [0], [a.BOT_PLAYER]), ("pool_level", [0], [1], [0.5]),
                         ("pool_open", [1], [1], [a.BOT_PLAYER]),
                         ("pool_open", [2], [2], [a.BOT_PLAYER]), ("pool_level", [2], [0], [1.0]),
                         ("pool_open", [3], [3], [a.BOT_PLAYER]), ("pool_level", [3], [0], [0.0])]
    assert (a.level, b.level, c.level, d.level) == (Level(3, 0.5, 1), None, Level(None, 1.0, 0), Level(2, 0.0, 0))
    del eng.calls[:]
    out = pool.move_bots([d, a, b])
    assert [x[0] for x in eng.calls] == ["pool_select_budget", "search", "lookup_dev", "step", "pool_hold", "counters"]
    assert eng.calls[0] == ("pool_select_budget", [d.slot, a.slot, b.slot], [2, 3, 5])
    assert eng.calls[1] == ("search", 5, 8)
    assert eng.calls[2] == ("lookup_dev", [d.slot, a.slot, b.slot])
    assert [o[1] for o in out] == [0.5] * 3 and all(s.value == 0.5 for s in (d, a, b)) and c.moves == []
    # the launches run to the largest budget LISTED, not to the pool's
    for s in (d, a):
        s.move_player(min(pool.game.possible_moves(s.state)))
    del eng.calls[:]
    pool.move_bots([a, d])
    assert eng.calls[0] == ("pool_select_budget", [a.slot, d.slot], [3, 2]) and eng.calls[1] == ("search", 3, 8)
    assert not any(x[0] in ("pool_level", "pool_select") for x in eng.calls)


def test_pool_level_goes_out_at_open_and_set_level_only():
    pool, eng = _pool()
    a, b = pool.open(True), pool.open(True, level=Level(4, 2.0))
    del eng.calls[:]
    a.move_player(3)
    b.move_player(2)
    pool.move_bots([a, b])
    assert not any(x[0] == "pool_level" for x in eng.calls)
    assert ("pool_select_budget", [a.slot, b.slot], [5, 4]) in eng.calls
    del eng.calls[:]
    b.set_level(Level(2, 0.0, 0))
    assert eng.calls == [("pool_level", [b.slot], [0], [0.0])] and b.level == Level(2, 0.0, 0)
    del eng.calls[:]
    b.set_level(None)  # back to the pool's own: the engine is told, levels are on
    assert eng.calls == [("pool_level", [b.slot], [0], [0.0])] and b.level is None
    del eng.calls[:]
    with pytest.raises(ValueError):
        b.set_level(Level(1))
    with pytest.raises(ValueError):
        b.set_level(Level(tau=0.01))
    assert eng.calls == [] and b.level is None
    pool.close(b)
    with pytest.raises(ValueError):
        b.set_level(Level(3))
    c = pool.open(True)  # b's slot again: pool_open alone puts it back to (net 0, tau 0)
    assert c.slot == b.slot and c.level is None and [x[0] for x in eng.calls] == ["pool_open"]
