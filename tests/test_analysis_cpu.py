"""Position analysis without a GPU: the two C symbols, the shared pick rule (caro_host_line_heads) against numpy, the
reference walker (tests/analysis_ref.py) on hand-written trees, and SessionPool.analyse / PooledSession.hint against a
stub engine that records the calls it gets and hands back canned arrays."""
import ctypes as C

import numpy as np
import pytest
import torch

from caro_ai_amd import _lib
from caro_ai_amd.lib.game.connect_four import ConnectFour
from caro_ai_amd.lib.game.tictactoe import TicTacToe
from caro_ai_amd.lib.session_pool import Analysis, Line, PooledSession, SessionPool
from tests import analysis_ref as ref
from tests.analysis_trees import c4_tree, ttt_tree

E_INVAL = -22


# ------------------------------------------------------------------ the symbols
def test_the_two_symbols_are_exported_and_refuse_null_arguments():
    L = _lib.load()
    for name in ("caro_principal_lines", "caro_host_line_heads"):
        assert hasattr(L, name) and name in _lib.EXPORTS
    assert L.caro_version() == 107
    buf = (C.c_int32 * 64)(0)  # (host memory: never read, the handle is refused first)
    p = C.cast(buf, C.c_void_p)
    assert L.caro_principal_lines(None, 1, p, 0, 1, 1, *([p] * 10), None) == E_INVAL
    assert L.caro_principal_lines(None, 0, None, 0, 3, 8, *([None] * 10), None) == E_INVAL
    assert b"null" in L.caro_last_error()
    assert L.caro_host_line_heads(7, None, 3, p) == E_INVAL
    assert L.caro_host_line_heads(7, p, 3, None) == E_INVAL
    for A, top in ((0, 3), (257, 3), (7, 0), (7, 17)):
        assert L.caro_host_line_heads(A, p, top, p) == E_INVAL, (A, top)
    bad = (C.c_int32 * 7)(1, -1, 0, 0, 0, 0, 0)
    assert L.caro_host_line_heads(7, C.cast(bad, C.c_void_p), 3, p) == E_INVAL


# ------------------------------------------------------------------ the pick rule
def _heads(N, top):
    N = np.ascontiguousarray(N, dtype=np.int32)
    out = np.full(top, 99, dtype=np.int32)
    n = _lib.load().caro_host_line_heads(len(N), N.ctypes.data, top, out.ctypes.data)
    return n, out.tolist()


def _want(N, top):
    """np.lexsort((arange, -N)) restricted to N > 0: N descending, action ascending"""
    N = np.asarray(N, dtype=np.int64)
    order = [int(a) for a in np.lexsort((np.arange(len(N)), -N)) if N[a] > 0][:top]
    return len(order), order + [-1] * (top - len(order))


@pytest.mark.parametrize("A", [7, 9, 225])
@pytest.mark.parametrize("top", [1, 3, 16])
def test_line_heads_rank_by_visits_then_action(A, top):
    rng = np.random.RandomState(1000 * A + top)
    for trial in range(40):
        N = rng.randint(0, 4, size=A)  # values 0 .. 3: ties everywhere
        if trial % 8 == 7:
            N[rng.rand(A) < 0.9] = 0   # a sparse row: fewer visited edges than `top`
        assert _heads(N, top) == _want(N, top), (A, top, N.tolist())
    assert _heads(np.zeros(A, np.int32), top) == (0, [-1] * top)
    one = np.zeros(A, np.int32)
    one[A - 1] = 5
    assert _heads(one, top) == (1, [A - 1] + [-1] * (top - 1))


def test_line_heads_first_is_argmax_and_large_counts_order():
    rng = np.random.RandomState(5)
    for A in (7, 9, 225):
        for _ in range(20):
            N = rng.randint(0, 3, size=A)
            n, heads = _heads(N, 1)
            assert (n, heads[0]) == ((1, int(np.argmax(N))) if N.max() > 0 else (0, -1))
    big = np.array([(1 << 30) - 1, 1, (1 << 30) - 1, (1 << 30) - 2, 0, 256, 255], dtype=np.int32)
    assert _heads(big, 16) == _want(big, 16) == (6, [0, 2, 3, 5, 6, 1] + [-1] * 10)
    assert _heads([2, 2, 2], 2) == (2, [0, 1])  # top smaller than the visited edges: the first `top` of the ranking


# ------------------------------------------------------------------ the reference walker, by hand
def _walk(game, nodes, root, top, depth):
    state, player = root
    got = ref.principal_lines(game, nodes.get, state, player, top, depth)
    return got["root_visits"], [([s["move"] for s in ln["steps"]], ref.END_NAMES[ln["end"]]) for ln in got["lines"]]


def test_the_reference_walker_on_a_hand_written_3x3_tree():
    game = TicTacToe(3, 3)
    nodes, roots = ttt_tree(game)
    # the tie at the root (0 before 8), the tie below it ([4]: 0 before 1), LEAF twice over, WIN, top > visited edges
    assert _walk(game, nodes, roots["open"], 16, 8) == (12, [([4, 0], "leaf"), ([0, 3, 1, 4, 2], "win"), ([8], "leaf"),
                                                            ([2], "leaf")])
    assert _walk(game, nodes, roots["open"], 3, 8)[1] == [([4, 0], "leaf"), ([0, 3, 1, 4, 2], "win"), ([8], "leaf")]
    # a line that reaches `depth` exactly on its winning move says WIN; one move short it says DEPTH
    assert _walk(game, nodes, roots["open"], 2, 5)[1] == [([4, 0], "leaf"), ([0, 3, 1, 4, 2], "win")]
    assert _walk(game, nodes, roots["open"], 2, 4)[1] == [([4, 0], "leaf"), ([0, 3, 1, 4], "depth")]
    assert _walk(game, nodes, roots["open"], 2, 2)[1] == [([4, 0], "depth"), ([0, 3], "depth")]
    # depth = 1: DEPTH comes before LEAF
    assert _walk(game, nodes, roots["open"], 4, 1) == (12, [([4], "depth"), ([0], "depth"), ([8], "depth"),
                                                           ([2], "depth")])
    # DRAW: the board fills up; it comes before DEPTH too
    assert _walk(game, nodes, roots["late"], 3, 8) == (3, [([6, 8], "draw"), ([8], "leaf")])
    assert _walk(game, nodes, roots["late"], 1, 2) == (3, [([6, 8], "draw")])
    assert _walk(game, nodes, roots["absent"], 3, 8) == (-1, [])
    # the recorded words are the edge's own
    got = ref.principal_lines(game, nodes.get, *roots["open"], 1, 2)
    root, child = nodes[roots["open"][0]], nodes[game.move(roots["open"][0], 4, 1)[0]]
    for step, (node, a) in zip(got["lines"][0]["steps"], ((root, 4), (child, 0))):
        assert step == {"move": a, "N": int(node["N"][a]), "W": float(node["W"][a]), "Q": float(node["Q"][a]),
                        "P": float(node["P"][a]), "strong": int(node["W_is_f32"][a])}


def test_the_reference_walker_on_a_hand_written_connect_four_tree():
    game = ConnectFour()
    nodes, roots = c4_tree(game)
    assert _walk(game, nodes, roots["open"], 3, 8) == (9, [([0, 1, 0, 1, 0, 1, 0], "win"), ([3, 3], "leaf"),
                                                          ([6], "leaf")])
    assert _walk(game, nodes, roots["open"], 1, 7)[1] == [([0, 1, 0, 1, 0, 1, 0], "win")]
    assert _walk(game, nodes, roots["open"], 1, 6)[1] == [([0, 1, 0, 1, 0, 1], "depth")]
    assert _walk(game, nodes, roots["absent"], 3, 8) == (-1, [])


# ------------------------------------------------------------------ SessionPool.analyse on a stub engine
class StubEngine:
    """what SessionPool.analyse asks of a SelfPlayEngine: records the calls, hands back canned read-out arrays"""

    def __init__(self, game, n):
        self.game, self.G = game, n
        self.calls = []
        self.overflows = 0
        self.canned = None  # slot -> (root_visits, [(moves, N, W, Q, P, strong, end code)])

        class Cfg:
            node_cap = 0
        self.cfg = Cfg()

    def pool_open(self, slots, uids, first_players):
        self.calls.append(("pool_open", list(slots)))

    def pool_set(self, slots, states, players, plies):
        self.calls.append(("pool_set", list(slots)))

    def pool_select(self, slots):
        self.calls.append(("pool_select", list(slots)))

    def search(self, searches, batch):
        self.calls.append(("search", searches, batch))

    def principal_lines(self, slots, top, depth, store=0):
        self.calls.append(("principal_lines", list(slots), top, depth, store))
        M = len(slots)
        # garbage beyond n_lines / len: analyse must trim, not trust the padding
        out = {"n_lines": torch.zeros(M, dtype=torch.int32), "root_visits": torch.full((M,), -1, dtype=torch.int32),
               "len": torch.full((M, top), 77, dtype=torch.int32), "end": torch.full((M, top), 2, dtype=torch.int32)}
        for k in ("move", "N", "strong"):
            out[k] = torch.full((M, top, depth), 9, dtype=torch.int32)
        for k in ("W", "Q", "P"):
            out[k] = torch.full((M, top, depth), 0.75)
        for i, g in enumerate(slots):
            visits, lines = (self.canned or {}).get(g, (-1, []))
            out["root_visits"][i] = visits
            out["n_lines"][i] = len(lines)
            for j, (moves, N, W, Q, P, strong, end) in enumerate(lines):
                n = len(moves)
                out["len"][i, j], out["end"][i, j] = n, end
                for k, vals in (("move", moves), ("N", N), ("W", W), ("Q", Q), ("P", P), ("strong", strong)):
                    out[k][i, j, :n] = torch.as_tensor(vals, dtype=out[k].dtype)
        return out

    def pool_hold(self):
        self.calls.append(("pool_hold",))

    def counters(self):
        self.calls.append(("counters",))
        return {"overflows": self.overflows}


def _pool(slots=4):
    game = ConnectFour()
    eng = StubEngine(game, slots)
    return SessionPool(game, "weights.dat", slots=slots, device="cpu", searches=5, batch=8, engine=eng), eng


def test_analyse_selects_the_listed_slots_reads_out_and_holds():
    pool, eng = _pool()
    a, b, c = pool.open(False), pool.open(True), pool.open(False)  # b: the human is to move -- analysed all the same
    del eng.calls[:]
    out = pool.analyse([c, b])
    assert [x[0] for x in eng.calls] == ["pool_select", "principal_lines", "pool_hold", "counters"]  # no search
    assert eng.calls[0] == ("pool_select", [c.slot, b.slot])
    assert eng.calls[1] == ("principal_lines", [c.slot, b.slot], 3, 8, 0)
    assert out == [Analysis(c.BOT_PLAYER, None, ()), Analysis(b.USER_PLAYER, None, ())]
    assert (a.moves, b.moves, c.moves) == ([], [], []) and a.state == pool.game.initial_state
    del eng.calls[:]
    pool.analyse([a], searches=2, top=5, depth=4)
    assert [x[0] for x in eng.calls] == ["pool_select", "search", "principal_lines", "pool_hold", "counters"]
    assert eng.calls[0] == ("pool_select", [a.slot]) and eng.calls[1] == ("search", 2, 8)
    assert eng.calls[2] == ("principal_lines", [a.slot], 5, 4, 0)


def test_analyse_builds_the_records_from_the_arrays():
    pool, eng = _pool()
    a, b = pool.open(False), pool.open(True)
    eng.canned = {
        a.slot: (11, [([3, 2, 4], [6, 4, 1], [1.5, -2.0, 1.0], [0.125, 0.625, 0.25], [0.5, 0.25, 0.125], [1, 0, 0], 0),
                      ([0], [5], [2.5], [0.375], [0.0625], [0], 3)]),
        b.slot: (4, [([6, 6], [3, 1], [0.75, 1.0], [-0.5, 0.875], [0.25, 0.5], [0, 1], 1),
                     ([1], [1], [0.0], [0.0], [0.5], [0], 2)]),
    }
    got_a, got_b = pool.analyse([a, b], top=4, depth=5)
    assert isinstance(got_a, Analysis) and isinstance(got_a.lines[0], Line)
    assert (got_a.to_move, got_a.root_visits, len(got_a.lines)) == (a.BOT_PLAYER, 11, 2)
    # trimmed to len; value = the float32 Q word where strong, else W / N
    assert got_a.lines[0] == Line((3, 2, 4), (6, 4, 1), (np.float32(0.125), -2.0 / 4, 1.0 / 1), (0.5, 0.25, 0.125),
                                  "depth")
    assert isinstance(got_a.lines[0].values[0], np.float32) and isinstance(got_a.lines[0].values[1], float)
    assert got_a.lines[1] == Line((0,), (5,), (2.5 / 5,), (0.0625,), "leaf")
    assert (got_b.to_move, got_b.root_visits) == (b.USER_PLAYER, 4)
    assert got_b.lines[0] == Line((6, 6), (3, 1), (0.75 / 3, np.float32(0.875)), (0.25, 0.5), "win")
    assert got_b.lines[1].end == "draw" and got_b.lines[1].values == (0.0,)
    with pytest.raises(AttributeError):  # plain immutable records
        got_a.root_visits = 3
    text = got_a.text().splitlines()
    assert len(text) == 2 and "3 2 4" in text[0] and "6" in text[0] and "+0.12" in text[0] and "+0.50" in text[1]
    assert isinstance(Analysis(0, None, ()).text(), str)
    # hint() is analyse([s])[0]
    del eng.calls[:]
    assert a.hint(top=4, depth=5) == got_a
    assert eng.calls[0] == ("pool_select", [a.slot]) and eng.calls[1] == ("principal_lines", [a.slot], 4, 5, 0)
    assert b.hint(searches=1)[0] == b.USER_PLAYER and ("search", 1, 8) in eng.calls
    assert isinstance(a, PooledSession)


def test_analyse_refuses_before_any_engine_call():
    pool, eng = _pool()
    other, _ = _pool()
    a, b = pool.open(False), pool.open(True)
    foreign = other.open(False)
    closed = pool.open(False)
    pool.close(closed)
    finished = pool.open(False)
    finished.finished = True
    del eng.calls[:]
    for bad in ([a, a], [a, closed], [foreign], [finished], [a, object()]):
        with pytest.raises(ValueError):
            pool.analyse(bad)
    with pytest.raises(ValueError):
        pool.analyse([a], searches=-1)
    with pytest.raises(ValueError):
        finished.hint()
    assert eng.calls == []
    assert pool.analyse([]) == [] and eng.calls == []
    assert pool.analyse([b, a]) and eng.calls[0] == ("pool_select", [b.slot, a.slot])  # either side may be to move
    eng.overflows = 1
    with pytest.raises(_lib.CaroError):  # an overflow is an error, exactly as in move_bots
        pool.analyse([a], searches=1)
    pool.analyse([a])  # ... reported once
