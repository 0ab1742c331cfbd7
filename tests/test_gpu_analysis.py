"""Position analysis on the GPU: caro_principal_lines against the pure-Python walker (tests/analysis_ref.py) on hand-built
trees and on searched ones (the oracle twin of every session), SessionPool.analyse read-only and pondering, the
read-only property at the C-ABI, and the refusals."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from caro_ai_amd.engine import SelfPlayEngine
from caro_ai_amd.lib.game.connect_four import ConnectFour
from caro_ai_amd.lib.game.tictactoe import TicTacToe
from caro_ai_amd.lib.session_pool import SessionPool
from caro_ai_amd.net_hip import HashNet
from tests import analysis_ref as ref
from tests.analysis_trees import c4_tree, ttt_tree

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED, SALT = 77, 5
E_INVAL, E_STATE = -22, -71
SENTINEL = -12345
FIELDS = (("n_lines", np.int32, 0), ("root_visits", np.int32, 0), ("len", np.int32, 1), ("end", np.int32, 1),
          ("move", np.int32, 2), ("N", np.int32, 2), ("W", np.float32, 2), ("Q", np.float32, 2), ("P", np.float32, 2),
          ("strong", np.int32, 2))  # (name, dtype, 0: [M] / 1: [M, top] / 2: [M, top, depth]) in the C argument order


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


def _engine(game, batch=8, **kw):
    return SelfPlayEngine(game, 8, evaluators=[HashNet(game, device=DEV, salt=SALT)], max_batch=batch, seed=SEED,
                          steps_before_tau_0=0, device=DEV, searches_hint=3, **kw)


def _raw(eng, slots, top, depth, store=0, M=None, null=None):
    """caro_principal_lines on buffers pre-filled with SENTINEL -> (return code, {name: numpy array})"""
    g = torch.tensor(list(slots) or [0], dtype=torch.int32, device=DEV)
    M = len(slots) if M is None else M
    rows = max(len(slots), 1)
    shape = {0: (rows,), 1: (rows, max(top, 1)), 2: (rows, max(top, 1), max(depth, 1))}
    bufs = {name: torch.full(shape[rank], SENTINEL, dtype=torch.from_numpy(np.zeros(1, dt)).dtype, device=DEV)
            for name, dt, rank in FIELDS}
    ptrs = [None if name == null else C.c_void_p(bufs[name].data_ptr()) for name, _, _ in FIELDS]
    rc = eng.L.caro_principal_lines(eng.h, M, None if null == "games" else C.c_void_p(g.data_ptr()), store, top, depth,
                                    *ptrs, eng._stream())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in bufs.items()}


def _untouched(out):
    return all(bool((a == SENTINEL).all()) for a in out.values())


def _compare(out, i, want, top, depth, tag, priors=True):
    """slot row i of a read-out against the walker's result, element for element, unused entries included: moves, N,
    len, end exact; strong == W_is_f32; W exact after the float64 cast; Q by the pool test's two-case rule"""
    lines = want["lines"]
    assert int(out["root_visits"][i]) == want["root_visits"], tag
    assert int(out["n_lines"][i]) == len(lines), tag
    for j in range(top):
        steps = lines[j]["steps"] if j < len(lines) else []
        n = len(steps)
        assert int(out["len"][i, j]) == n, (tag, j)
        assert int(out["end"][i, j]) == (lines[j]["end"] if j < len(lines) else -1), (tag, j)
        assert out["move"][i, j].tolist() == [s["move"] for s in steps] + [-1] * (depth - n), (tag, j)
        assert out["N"][i, j].tolist() == [s["N"] for s in steps] + [0] * (depth - n), (tag, j)
        assert out["strong"][i, j].tolist() == [s["strong"] for s in steps] + [0] * (depth - n), (tag, j)
        assert out["W"][i, j].astype(np.float64).tolist() == [s["W"] for s in steps] + [0.0] * (depth - n), (tag, j)
        for d, s in enumerate(steps):
            if s["strong"]:
                assert float(out["Q"][i, j, d]) == s["Q"], (tag, j, d)
            else:
                assert np.float32(s["Q"]) == out["Q"][i, j, d], (tag, j, d)
            if priors:
                assert np.float32(s["P"]) == out["P"][i, j, d], (tag, j, d)
        assert not out["Q"][i, j, n:].any() and not out["P"][i, j, n:].any(), (tag, j)


def _check_analysis(an, want, to_move, tag):
    """an Analysis record against the walker's result: values[d] is the edge's Q as get_node reports it"""
    assert an.to_move == to_move, tag
    assert an.root_visits == (None if want["root_visits"] < 0 else want["root_visits"]), tag
    assert len(an.lines) == len(want["lines"]), tag
    for ln, w in zip(an.lines, want["lines"]):
        assert list(ln.moves) == [s["move"] for s in w["steps"]], tag
        assert list(ln.visits) == [s["N"] for s in w["steps"]], tag
        assert ln.end == ref.END_NAMES[w["end"]], tag
        assert [float(v) for v in ln.values] == [s["Q"] for s in w["steps"]], tag


# ------------------------------------------------------------------ hand-built trees
def _poke(eng, slots, nodes):
    """every node of `nodes` into tree (slot, 0) of each listed slot"""
    game = eng.game
    states = list(nodes) * len(slots)
    g = torch.tensor([s for s in slots for _ in nodes], dtype=torch.int32, device=DEV)
    z = torch.zeros_like(g)
    keys = torch.from_numpy(game.to_keys(states).view(np.int64)).to(DEV)
    cols = [np.stack([nodes[s][k] for s in states]).astype(dt) for k, dt in
            (("N", np.int32), ("W", np.float32), ("Q", np.float32), ("P", np.float32), ("W_is_f32", np.int32))]
    t = [torch.from_numpy(np.ascontiguousarray(c)).to(DEV) for c in cols]
    assert eng.L.caro_poke_nodes(eng.h, len(states), C.c_void_p(g.data_ptr()), C.c_void_p(z.data_ptr()),
                                 C.c_void_p(keys.data_ptr()), *[C.c_void_p(x.data_ptr()) for x in t],
                                 eng._stream()) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["ttt3", "c4"])
def test_hand_built_trees_read_out_as_the_walker_walks_them(name):
    game, build = (TicTacToe(3, 3), ttt_tree) if name == "ttt3" else (ConnectFour(), c4_tree)
    nodes, roots = build(game)
    eng = _engine(game)
    names = sorted(roots)  # one slot per root, each with the whole tree poked into its own store
    _poke(eng, list(range(len(names))), nodes)
    plies = {"open": 0, "late": 7, "absent": 2}
    eng.pool_set(list(range(len(names))), [roots[k][0] for k in names], [roots[k][1] for k in names],
                 [plies[k] for k in names])
    listed = list(range(len(names))) + [0]  # a slot may be listed twice
    ends, lens = set(), set()
    for top, depth in ((16, 8), (3, 8), (2, 5), (2, 4), (1, 7), (1, 6), (4, 1), (1, 2), (16, 64)):
        rc, out = _raw(eng, listed, top, depth)
        assert rc == 0
        for a in out.values():
            assert not (a == SENTINEL).any(), (name, top, depth)  # every element was written, unused ones included
        for i, g in enumerate(listed):
            k = names[g]
            want = ref.principal_lines(game, nodes.get, roots[k][0], roots[k][1], top, depth)
            _compare(out, i, want, top, depth, (name, k, top, depth))
            ends |= {(k, top, depth, ln["end"]) for ln in want["lines"]}
            lens |= {(k, top, depth, j, len(ln["steps"])) for j, ln in enumerate(want["lines"])}
        for f in out:  # the twice-listed slot: the same rows twice
            assert np.array_equal(out[f][0], out[f][-1]), f
        i_open, i_absent = names.index("open"), names.index("absent")
        assert out["n_lines"][i_absent] == 0 and out["root_visits"][i_absent] == -1  # a root that is no node
        assert out["n_lines"][i_open] == min(top, 4 if name == "ttt3" else 3)         # top > visited root edges
    # what the trees were built to show did occur (the walker's own results are pinned in tests/test_analysis_cpu.py)
    if name == "ttt3":
        assert {e[3] for e in ends} == {ref.WIN, ref.DRAW, ref.DEPTH, ref.LEAF}
        assert ("open", 2, 5, ref.WIN) in ends and ("open", 2, 5, 1, 5) in lens   # depth reached on the winning move
        assert ("open", 2, 4, ref.DEPTH) in ends and ("late", 1, 2, ref.DRAW) in ends
        assert ("open", 4, 1, ref.DEPTH) in ends and ("open", 4, 1, 3, 1) in lens  # depth = 1
        rc, out = _raw(eng, [names.index("open")], 3, 8)
        assert out["move"][0, :, 0].tolist() == [4, 0, 8]  # the tie at the root: 0 before 8
        assert out["move"][0, 0, :2].tolist() == [4, 0]    # the tie below it: 0 before 1
    else:
        assert {e[3] for e in ends} == {ref.WIN, ref.DEPTH, ref.LEAF}
        assert ("open", 1, 7, ref.WIN) in ends and ("open", 1, 7, 0, 7) in lens and ("open", 1, 6, ref.DEPTH) in ends
        rc, out = _raw(eng, [names.index("open")], 3, 8)
        assert out["move"][0, :, 0].tolist() == [0, 3, 6] and out["move"][0, 1, :2].tolist() == [3, 3]
    eng.close()


# ------------------------------------------------------------------ searched trees, against the oracle
GEOMETRIES = [
    ("c4-b8-k_tree", lambda: ConnectFour(), 8, False, None),
    ("c4-b4-dense", lambda: ConnectFour(), 4, False, None),
    ("ttt3-b8-k_tree_mw", lambda: TicTacToe(3, 3), 8, False, None),
    ("caro15-b8-k_tree_mw-evict", lambda: _caro(15, 5), 8, True, 1024),
]
OPENS = {0: [True, False], 1: [False], 2: [True], 4: [False, True]}  # round -> sessions opened (True: the human moves first)
CLOSES = {3: [0, 1]}
ROUNDS = 9
TOP, DEPTH = 3, 6


def _analyse_and_check(pool, twins, sessions, listed, searches, tag, seen):
    """analyse(listed) against the walker over each session's twin, and the raw read-out of the same slots"""
    game, eng = pool.game, pool.engine
    if searches:
        for s in listed:
            twins[sessions.index(s)].search_batch(searches, pool.batch, s.state, s.to_move, ply=len(s.moves))
    got = pool.analyse(listed, searches=searches, top=TOP, depth=DEPTH)
    raw = {k: v.cpu().numpy() for k, v in eng.principal_lines([s.slot for s in listed], TOP, DEPTH).items()}
    for i, s in enumerate(listed):
        o = twins[sessions.index(s)]
        want = ref.principal_lines(game, o.get_node, s.state, s.to_move, TOP, DEPTH)
        _check_analysis(got[i], want, s.to_move, (tag, s.uid, len(s.moves)))
        _compare(raw, i, want, TOP, DEPTH, (tag, s.uid, len(s.moves)), priors=False)
        seen["bot" if s.to_move == s.BOT_PLAYER else "human"] += 1
        seen["unsearched"] += want["root_visits"] < 0
        seen["long"] += any(len(ln["steps"]) >= 2 for ln in want["lines"])
        seen["lines"] += len(want["lines"]) >= 1
        seen["ranked"] += len(want["lines"]) >= 2
    return got


def _bots_move_as_their_twins(pool, twins, sessions, pick, S, tag):
    before = [(s.state, len(s.moves)) for s in pick]
    out = pool.move_bots(pick)
    for s, (state, ply), (move, value, won) in zip(pick, before, out):
        o = twins[sessions.index(s)]
        o.search_batch(S, pool.batch, state, s.BOT_PLAYER, ply=ply)
        node = o.get_node(state)
        assert move == int(np.argmax(o.get_policy(state, tau=0))), (tag, s.uid, ply)
        assert value == node["Q"][move], (tag, s.uid, ply, value, node["Q"][move])


def _play(name, make_game, batch, evict, node_cap, ponder):
    """the session pool test's schedule; every round every open unfinished session is analysed, on human turns and on bot
    turns -- read-only (ponder = False), or with S searches on the human turns and on the first bot turn of each session"""
    game = make_game()
    S = 3
    pool = _pool(game, batch, evict=evict, node_cap=node_cap, searches=S)
    rng = random.Random(20261019)
    sessions, twins, pondered_bot = [], [], set()
    seen = {"bot": 0, "human": 0, "unsearched": 0, "long": 0, "lines": 0, "ranked": 0}
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
        live = [s for s in sessions if not s.closed and not s.finished]
        if not ponder:
            _analyse_and_check(pool, twins, sessions, live, 0, (name, rnd), seen)
        else:
            humans = [s for s in live if s.to_move == s.USER_PLAYER]
            if humans:
                _analyse_and_check(pool, twins, sessions, humans, S, (name, rnd, "human"), seen)
        for s in live:
            if s.to_move == s.USER_PLAYER:
                s.move_player(rng.choice(game.possible_moves(s.state)))
        live = [s for s in live if not s.finished]
        if ponder:  # one pondered bot turn per session: a second search of the same ply and position follows it
            fresh = [s for s in live if s.bots_turn() and s.uid not in pondered_bot]
            if fresh:
                _analyse_and_check(pool, twins, sessions, fresh, S, (name, rnd, "bot"), seen)
                pondered_bot |= {s.uid for s in fresh}
        elif live:
            _analyse_and_check(pool, twins, sessions, live, 0, (name, rnd, "after the human"), seen)
        ready = [s for s in sessions if s.bots_turn()]
        pick = ready if rnd % 3 == 0 else ready[:1] if rnd % 3 == 1 else ready[::-2]
        if pick:
            _bots_move_as_their_twins(pool, twins, sessions, pick, S, (name, rnd))
    assert len(sessions) == 6 and seen["human"] and seen["bot"] and seen["lines"], seen
    # read-only at 3 x 8 simulations a kept tree is too thin below the root's children for a second step (an edge there
    # needs two visits through its parent): those runs show unsearched roots and one-step lines, pondering the long ones
    assert (seen["long"] and seen["ranked"]) if ponder else seen["unsearched"], seen
    print(name, "ponder" if ponder else "read-only", seen)
    assert pool.engine.counters()["overflows"] == 0 and pool.engine.pending_leaves() == 0
    pool.close_pool()


@pytest.mark.parametrize("name,make_game,batch,evict,node_cap", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_analysis_of_searched_trees_is_the_walk_over_the_oracle_twin(name, make_game, batch, evict, node_cap):
    """searches = 0 on human turns and on bot turns: the lines are the walker's over the twin's kept store, and the bot's
    moves and values throughout are still the twin's -- the analysis changed nothing"""
    _play(name, make_game, batch, evict, node_cap, ponder=False)


@pytest.mark.parametrize("name,make_game,batch,evict,node_cap", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_pondering_keeps_its_visits_and_the_twin_follows(name, make_game, batch, evict, node_cap):
    """searches = S on human turns and on one bot turn of each session: the twin runs the same search_batch at the same
    points (the sim index of the noise key restarts at 0 in both), lines, later moves and values stay equal"""
    _play(name, make_game, batch, evict, node_cap, ponder=True)


def test_pondering_on_the_bots_turn_finds_the_move_move_bots_makes():
    game = ConnectFour()
    S, B = 3, 8
    a, b = _pool(game, B, searches=S), _pool(game, B, searches=S)
    rng = random.Random(8)
    sa, sb = a.open(True, uid=5), b.open(True, uid=5)
    for turn in range(3):
        move = rng.choice(game.possible_moves(sa.state))
        sa.move_player(move)
        sb.move_player(move)
        if turn < 2:  # two plies of common history, no analysis in either pool
            assert a.move_bots([sa]) == b.move_bots([sb])
    got = sa.hint(searches=S)
    (move, value, won), = b.move_bots([sb])
    assert got.lines[0].moves[0] == move and got.lines[0].values[0] == value
    assert got.to_move == sa.BOT_PLAYER and got.root_visits > 0
    assert "visits" in got.text()
    a.close_pool()
    b.close_pool()


# ------------------------------------------------------------------ read-only
def test_the_read_out_changes_nothing_and_pondering_leaves_the_other_slots_alone():
    game = ConnectFour()
    S, B = 3, 8
    pool = _pool(game, B, searches=S)
    eng = pool.engine
    rng = random.Random(3)
    sessions = [pool.open(i % 2 == 0) for i in range(6)]
    for _ in range(2):
        for s in sessions:
            if s.to_move == s.USER_PLAYER:
                s.move_player(rng.choice(game.possible_moves(s.state)))
        pool.move_bots([s for s in sessions if s.bots_turn()])

    def snapshot():
        rows = eng.lookup([s.slot for s in sessions], [0] * len(sessions), [s.state for s in sessions])
        return eng.roots() + (eng.tree_sizes(), eng.tree_live(), sorted(eng.counters().items())) + \
            tuple(rows[k] for k in sorted(rows))

    s0 = snapshot()
    rc, out = _raw(eng, list(range(eng.G)) + [2, 2], 3, 8)  # every slot: sessions' and never-opened ones, one twice more
    assert rc == 0 and not any((a == SENTINEL).any() for a in out.values())
    assert out["n_lines"].max() >= 1 and out["root_visits"][6:8].tolist() == [-1, -1]
    s1 = snapshot()
    for x, y in zip(s0, s1):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
    assert eng.live_games() == 0 and eng.pending_leaves() == 0
    # pondering two sessions: the held slots that are not listed keep every word
    subset = [sessions[1], sessions[4]]
    others = [g for g in range(eng.G) if g not in (subset[0].slot, subset[1].slot)]
    rows0 = eng.lookup(others[:4], [0] * 4, [sessions[g].state for g in others[:4]])
    c0 = eng.counters()
    pool.analyse(subset, searches=S)
    s2 = snapshot()
    for x, y in zip(s0[:6], s2[:6]):  # keys, players, plies, uids, tree sizes, live nodes
        assert np.array_equal(x[others], y[others])
    for x, y in zip(s0[:4], s2[:4]):  # the pondered slots keep their position, mover, ply and uid
        assert np.array_equal(x, y)
    rows1 = eng.lookup(others[:4], [0] * 4, [sessions[g].state for g in others[:4]])
    for k in rows0:
        assert np.array_equal(rows0[k], rows1[k]), k
    c1 = eng.counters()
    assert c1["sims"] - c0["sims"] == S * B * len(subset) and c1["plies"] == c0["plies"]
    assert eng.live_games() == 0 and eng.pending_leaves() == 0 and c1["overflows"] == 0
    pool.close_pool()


# ------------------------------------------------------------------ refusals
def test_the_read_out_refuses_what_it_must():
    game = ConnectFour()
    S, B = 3, 8
    stag = SelfPlayEngine(game, 8, evaluators=[HashNet(game, device=DEV, salt=SALT)], max_batch=B, seed=SEED,
                          device=DEV, searches_hint=S, stagger=True)
    rc, out = _raw(stag, [0], 3, 8)
    assert rc == E_STATE and _untouched(out)
    stag.close()

    eng = _engine(game, B)
    eng.search(S, B)
    st = eng._stream()
    bad = [dict(slots=[8]), dict(slots=[0, -1]), dict(slots=[1 << 20, 0]), dict(slots=[0], M=-1),
           dict(slots=[0], store=1), dict(slots=[0], store=-1), dict(slots=[0], top=0), dict(slots=[0], top=17),
           dict(slots=[0], depth=0), dict(slots=[0], depth=65), dict(slots=[0], null="games")]
    bad += [dict(slots=[0], null=name) for name, _, _ in FIELDS]
    for kw in bad:
        args = dict(top=3, depth=8)
        args.update(kw)
        rc, out = _raw(eng, args.pop("slots"), args.pop("top"), args.pop("depth"), **args)
        assert rc == E_INVAL and _untouched(out), kw
    p = C.c_void_p(eng.planes.data_ptr())
    assert eng.L.caro_principal_lines(None, 1, p, 0, 3, 8, *([p] * 10), st) == E_INVAL
    rc, out = _raw(eng, [], 3, 8)
    assert rc == 0 and _untouched(out)  # M == 0: nothing to do
    # the engine goes on working, and the accepted call reads the searched roots
    rc, out = _raw(eng, [7, 0], 16, 64)
    assert rc == 0 and not any((a == SENTINEL).any() for a in out.values())
    assert out["root_visits"].min() >= 1 and out["n_lines"].min() >= 1
    eng.step()
    c = eng.counters()
    assert c["sims"] == 8 * S * B and c["plies"] == 8 and c["overflows"] == 0
    # a select is pending: refused, and accepted again once it is dropped
    assert eng.L.caro_select(eng.h, B, 0, None, p, C.c_void_p(eng.leaf_keys.data_ptr()), st) == 0
    rc, out = _raw(eng, [0], 3, 8)
    assert rc == E_STATE and _untouched(out)
    assert eng.L.caro_select_cancel(eng.h) == 0
    rc, out = _raw(eng, [0], 3, 8)
    assert rc == 0
    eng.close()
