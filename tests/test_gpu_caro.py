"""Caro (blocked-five gomoku, CARO_GAME_CARO) on the GPU: the C-ABI's limits, the batched rule kernels and the tree
kernels (CaroRules instantiations) against the transitions and whole games recorded from the reference's search
driven by the caro rule (tests/golden/make_golden_caro.py), 1 024 concurrent games in both schedules against a
restatement of the rule, and the train / play command lines with `-g 2`."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import test_gpu_engine as tge
from tests.conftest import load_golden
from tests.test_caro_cpu import numpy_caro_won

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _caro(n, k):
    from caro_ai_amd.lib.game.caro import Caro
    return Caro(n, k)


@pytest.fixture(params=tge.FORMS)
def form(request):
    return request.param


def test_engine_create_limits():
    from caro_ai_amd import _lib
    L = _lib.load()
    h = C.c_void_p()

    def cfg(**kw):
        c = _lib.CaroConfig()
        c.game_kind, c.n, c.k, c.n_games, c.n_stores, c.n_nets, c.max_batch, c.node_cap = 2, 9, 5, 4, 1, 1, 8, 64
        c.c_puct, c.alpha, c.explore = 1.0, 0.3, 0.25
        for a, b in kw.items():
            setattr(c, a, b)
        return c

    for bad in (dict(n=16, k=5), dict(n=9, k=1), dict(n=9, k=10), dict(n=1, k=1), dict(n=15, k=16)):
        c = cfg(**bad)
        assert L.caro_engine_create(C.byref(c), C.byref(h)) == -22, bad  # CARO_E_INVAL
        assert L.caro_last_error()
    for ok in (dict(), dict(n=15, k=5), dict(n=4, k=4), dict(n=3, k=3, max_batch=4)):
        c = cfg(**ok)
        assert L.caro_engine_create(C.byref(c), C.byref(h)) == 0, (ok, L.caro_last_error())
        L.caro_engine_destroy(h)


def test_rules_kernels_vs_reference_recorded_transitions():
    """caro_rules_{legal,move,encode}_batch on every rules_caro transition: legal moves, next state, the caro result,
    and the planes TicTacToe's host helper gives (the caro board is the m,n,k board)"""
    from caro_ai_amd import _lib
    from caro_ai_amd.lib.game.tictactoe import TicTacToe
    L = _lib.load()
    d = load_golden("rules_caro.json.gz")
    differ = 0
    for b in d["boards"]:
        game, ttt = _caro(b["n"], b["k"]), TicTacToe(b["n"], b["k"])
        recs = b["recs"]
        M, A, HW = len(recs), game.action_space, b["n"] * b["n"]
        states = [int(r["s"]) for r in recs]
        keys = torch.from_numpy(game.to_keys(states).view(np.int64)).to(DEV)
        moves = torch.tensor([r["m"] for r in recs], dtype=torch.int32, device=DEV)
        players = torch.tensor([r["p"] for r in recs], dtype=torch.int32, device=DEV)
        legal = torch.zeros((M, A), dtype=torch.uint8, device=DEV)
        _lib.check(L.caro_rules_legal_batch(game.kind, game.n, game.k, M, keys.data_ptr(), legal.data_ptr(), None))
        won = torch.zeros(M, dtype=torch.int32, device=DEV)
        full = torch.zeros(M, dtype=torch.int32, device=DEV)
        _lib.check(L.caro_rules_move_batch(game.kind, game.n, game.k, M, keys.data_ptr(), moves.data_ptr(),
                                           players.data_ptr(), won.data_ptr(), full.data_ptr(), None))
        who = (1 - players).contiguous()
        planes = torch.zeros((M, 2 * HW), dtype=torch.float32, device=DEV)
        _lib.check(L.caro_rules_encode_batch(game.kind, game.n, game.k, M, keys.data_ptr(), who.data_ptr(),
                                             planes.data_ptr(), None))
        torch.cuda.synchronize()
        legal, won, planes = legal.cpu().numpy(), won.cpu().numpy(), planes.cpu().numpy()
        new_states = game.from_keys(keys.cpu().numpy().view(np.uint64))
        want_planes = ttt.states_to_training_batch([int(r["s2"]) for r in recs], [1 - r["p"] for r in recs])
        for i, r in enumerate(recs):
            assert np.flatnonzero(legal[i]).tolist() == ttt.possible_moves(states[i])
            assert str(new_states[i]) == r["s2"]
            assert bool(won[i]) == r["caro"], (b["n"], i)
            differ += r["caro"] != r["gomoku"]
        assert np.array_equal(planes.reshape(want_planes.shape), want_planes)
    assert differ >= 200


def _replay(g, form, **kw):
    tge._play_and_check_golden({"kind": "caro", "n": g["n"], "k": g["k"]}, g, form, **kw)


def test_engine_replays_reference_caro_games(form):
    """every synth_caro game but the 50 x 8 one, bit for bit: root N / W / Q / dtype flag, node count, pi, z, result
    (ref lib/mcts.py, lib/utils.py:25-108 with the caro win test)"""
    d = load_golden("synth_caro.json.gz")
    games = [g for g in d["games"] if g["searches"] != 50]
    assert {(g["n"], g["k"]) for g in games} == {(7, 4), (9, 5), (15, 5)}
    for g in games:
        _replay(g, form)


def test_engine_replays_reference_caro_game_400_sims_with_eviction(form):
    """the 15 x 15 game at config 4's 50 x 8 with eviction and a 4 096-node cap"""
    d = load_golden("synth_caro.json.gz")
    games = [g for g in d["games"] if g["searches"] == 50]
    assert len(games) == 1 and games[0]["n"] == 15
    _replay(games[0], form, node_cap=4096, evict=True)


# ------------------------------------------------------------------ tree search (CaroRules::move_group) vs the oracle
@pytest.mark.parametrize("n,k,B,two_nets", [(4, 2, 4, False), (4, 3, 4, False), (4, 4, 4, True),  # 16 lanes x 4
                                            (5, 3, 2, False), (5, 5, 2, False),                  # 32 x 2
                                            (8, 4, 1, False),                                    # 64 x 1
                                            (10, 5, 1, False), (11, 6, 1, False),                # 2 actions / lane
                                            (13, 5, 1, False)])                                  # 4 actions / lane
def test_caro_geometries_vs_oracle(n, k, B, two_nets, form):
    """every caro lane geometry, one wavefront per game (form=fused: k_tree), whole games recycled: every game equals
    the oracle's.  4 x 4 on 16 lanes is the one geometry whose lines fill their NL = 4 bits, so a run there reaches
    the seam between two lines of the ballot word (move_group's SEAM / inner masks); with k = 2 a blocked run fits"""
    S = 24 // B if n <= 5 else 10
    tge._check_against_oracle({"kind": "caro", "n": n, "k": k}, 8, 16 if n <= 5 else 8, 2, S, B, 2 if two_nets else 1,
                              seed=180 + n + k, uid_base=900, form=form, salts=(9, 10) if two_nets else None)


def test_caro_several_wavefronts_per_game_vs_oracle(form):
    """batch x lanes > 64 (dense rows in the fused form) on the seam geometry, and two nets with one store per
    player on 6 x 6 k 3"""
    tge._check_against_oracle({"kind": "caro", "n": 4, "k": 2}, 8, 16, 2, 6, 8, 1, seed=190, uid_base=0, form=form)
    tge._check_against_oracle({"kind": "caro", "n": 6, "k": 3}, 6, 8, 1, 5, 8, 2, seed=191, uid_base=50, form=form,
                              salts=(0x1111, 0x2222))


@pytest.mark.parametrize("d,B", [({"kind": "caro", "n": 4, "k": 3}, 4), ({"kind": "caro", "n": 4, "k": 2}, 8),
                                 ({"kind": "caro", "n": 7, "k": 4}, 1)])
def test_caro_staggered_vs_oracle(d, B):
    """the staggered schedule (k_tree_stag one wavefront per game, k_tree_stag_mw several) on caro boards, slots
    recycled: every game equals the oracle's"""
    tge._check_against_oracle(d, 8, 16, 2, 6, B, 1, seed=200 + B, uid_base=70, form="fused", stagger=True,
                              searches_hint=6)


def test_caro_eviction_vs_oracle(form):
    tge._check_evict({"kind": "caro", "n": 4, "k": 2}, 16, 24, 2, 12, 4, 1, seed=210, uid_base=0, cap=96, form=form)
    tge._check_evict({"kind": "caro", "n": 9, "k": 4}, 4, 4, 4, 6, 8, 1, seed=211, uid_base=0, cap=256, form=form)


def _caro_roots(n, k, limit):
    """search roots for the mover from tests/rules_cases.py: one move makes a blocked k (caro: no win, m,n,k: a win)
    and, where a second hand-built run fits beside it, another move makes an open k; on boards too small for a
    blocked k (n < k + 2) roots with an open k.  Returns [(cells, player)]"""
    from oracle.oracle import Oracle
    from tests.rules_cases import hand_built_cases
    o, t = Oracle(Oracle.CARO, n, k), Oracle(Oracle.MNK, n, k)

    def wins(b, m, p):
        return o.move_cells(b, m, p)[1], t.move_cells(b, m, p)[1]

    cases = hand_built_cases(n, k)
    blocked = [c for c in cases if wins(*c) == (False, True)]
    open_ = [c for c in cases if wins(*c) == (True, True)]
    rng = np.random.default_rng(100 * n + k)
    roots = []
    for b, m, p in (blocked or open_):
        root = b.copy()
        for j in rng.permutation(len(open_))[:8]:
            b2, m2, p2 = open_[j]
            if p2 != p or m2 == m:
                continue
            r = root.copy()
            free = (r == 2) & (b2 != 2)
            r[free] = b2[free]
            r[m2] = 2
            if wins(r, m, p) == wins(b, m, p) and wins(r, m2, p)[0]:
                root = r
                break
        if (root == 2).all() or (root != 2).all():
            continue
        roots.append((root, p))
    idx = np.sort(rng.permutation(len(roots))[:limit])
    return [roots[i] for i in idx]


@pytest.mark.parametrize("n,k,S,B,min_hits", [(3, 2, 6, 4, 0), (4, 2, 6, 4, 6), (4, 3, 6, 4, 0), (5, 3, 12, 2, 6),
                                              (8, 4, 24, 1, 10), (8, 5, 10, 8, 10), (11, 5, 10, 8, 10),
                                              (15, 5, 12, 8, 12)])
def test_caro_search_from_hand_built_roots(n, k, S, B, min_hits, form):
    """one slot per hand-built root (_caro_roots), S x B sims on empty trees: root N / W / Q / strong flag / tree size
    / pi equal the oracle's.  `min_hits` roots at least searched a child where the caro and the m,n,k rules part (a
    blocked k: not terminal under caro), so the blocked branch of move_group ran inside the tree kernels"""
    from oracle.oracle import Oracle
    roots = _caro_roots(n, k, 160)
    o, t = Oracle(Oracle.CARO, n, k), Oracle(Oracle.MNK, n, k)
    recs = [{"s2": str(o.to_int(b)), "p": 1 - p} for b, p in roots]
    counts = []
    checked, _ = tge._search_from_positions({"kind": "caro", "n": n, "k": k}, recs, S, B, seed=230 + n, form=form,
                                            root_counts=counts)
    assert checked == len(roots) >= 16
    hits = 0
    for (b, p), N in zip(roots, counts):
        for a in np.flatnonzero((b == 2) & (N > 0)):
            after = b.copy()
            after[a] = p
            r, c = divmod(int(a), n)
            if numpy_caro_won(after.reshape(n, n), r, c, k, p) != t.move_cells(b, a, p)[1]:
                hits += 1
                break
    assert hits >= min_hits, hits
    if n < k + 2:
        assert hits == 0


def _check_record(game, n, k, states, players, result, steps):
    """one finished game's replay rows (forward order): each move is the one cell that changes, no earlier ply was a
    caro win under the restatement, the last one is a caro win (result != 0) or fills the board (a draw)"""
    boards = [np.array(list(str(s).rjust(n * n, "0")), dtype=np.int8).reshape(n, n) for s in states]
    assert len(boards) == steps + 1
    for i, b in enumerate(boards):
        assert int(players[i]) == (int(players[0]) + i) % 2
        if i + 1 < len(boards):
            diff = np.argwhere(boards[i + 1] != b)
            assert len(diff) == 1 and b[tuple(diff[0])] == 2
            r, c = diff[0]
            assert boards[i + 1][r, c] == players[i]
            assert not numpy_caro_won(boards[i + 1], r, c, k, int(players[i])), i
    # the last move is not in the rows (the replay holds states before each move): it is one of the empty cells
    last, p = boards[-1], int(players[-1])
    if result == 0:
        assert (last == 2).sum() == 1
        return False
    wins = []
    for r, c in np.argwhere(last == 2):
        b = last.copy()
        b[r, c] = p
        wins.append(numpy_caro_won(b, r, c, k, p))
    assert any(wins)
    return True


def _rows_by_game(tuples, games):
    """split the drained rows into games: each game's rows come newest first, as play_game's replay buffer"""
    keys = np.concatenate([t["states"] for t in tuples]).view(np.uint64)
    players = np.concatenate([t["players"] for t in tuples])
    pi = np.concatenate([t["pi"] for t in tuples])
    z = np.concatenate([t["z"] for t in tuples])
    out, off = {}, 0
    for uid, first, result, steps in games.tolist():
        n = steps + 1
        out[uid] = (first, result, steps, keys[off:off + n][::-1], players[off:off + n][::-1], pi[off:off + n],
                    z[off:off + n])
        off += n
    assert off == len(z)
    return out


def test_1024_concurrent_caro_games_staggered_and_lock_step():
    """1 024 slots of 9 x 9 caro (k = 5), table net on the device, one game per slot: the staggered schedule and the
    lock-step one play the same 1 024 games (every row of every game equal), and every game is a legal caro game
    under the numpy restatement of the rule"""
    n, k, G, S, B, seed = 9, 5, 1024, 3, 8, 5
    game = _caro(n, k)
    runs = []
    for stagger in (False, True):
        eng = tge._engine(game, G, [tge._synth(game, "fused")], max_batch=B, steps_before_tau_0=81, seed=seed,
                          uid_base=0, stagger=stagger, stagger_recycle=False, searches_hint=S)
        tuples, games = eng.play_until(S, B, recycle=False, max_moves=1000)
        c = eng.counters()
        assert eng.live_games() == 0
        eng.close()
        assert c["overflows"] == 0 and sorted(games[:, 0].tolist()) == list(range(G))
        runs.append(_rows_by_game(tuples, games))
    lock, stag = runs
    wins = 0
    for uid in range(G):
        a, b = lock[uid], stag[uid]
        assert a[:3] == b[:3], uid
        for x, y in zip(a[3:], b[3:]):
            assert np.array_equal(x, y), uid
        first, result, steps, keys, players = a[:5]
        wins += _check_record(game, n, k, game.from_keys(keys), players, result, steps)
    assert wins > G // 2


def test_caro_3x3_is_tictactoe_at_1024_slots():
    """Caro(3, 3) and TicTacToe(3, 3), 1 024 slots, same seed: the same drained tuples, row for row"""
    from caro_ai_amd.lib.game.tictactoe import TicTacToe
    out = []
    for game in (_caro(3, 3), TicTacToe(3, 3)):
        eng = tge._engine(game, 1024, [tge._synth(game, "fused")], max_batch=8, steps_before_tau_0=4, seed=3,
                          uid_base=0, stagger=True, searches_hint=5)
        tuples, games = eng.play_until(5, 8, n_finished=3000)
        c = eng.counters()
        eng.close()
        assert c["overflows"] == 0
        out.append((games, tuples))
    (g1, t1), (g2, t2) = out
    assert np.array_equal(g1, g2)
    assert len(t1) == len(t2)
    for a, b in zip(t1, t2):
        assert a.keys() == b.keys()
        for key in a:
            assert np.array_equal(a[key], b[key]), key


def test_train_and_play_command_lines_with_caro(tmp_path, monkeypatch):
    """`train -g 2 ... --iterations 2` writes a checkpoint the Net loads; `play -g 2` runs two of them"""
    from caro_ai_amd import config as cfg
    from caro_ai_amd import play, train
    from caro_ai_amd.lib.model import Net
    monkeypatch.setattr(cfg, "MIN_REPLAY_TO_TRAIN", 300)
    monkeypatch.setattr(cfg, "EVALUATE_EVERY_STEP", 1)
    monkeypatch.setattr(cfg, "BEST_NET_WIN_RATIO", -1.0)  # always promote: a checkpoint per iteration
    monkeypatch.setattr(cfg, "EVALUATION_ROUNDS", 2)
    monkeypatch.setattr(cfg, "BATCH_SIZE", 32)
    monkeypatch.setattr(cfg, "TRAIN_ROUNDS", 2)
    train.release_engines()
    train.main(["-n", "caro", "-g", "2", "--cuda", "--games", "16", "--iterations", "2", "--saves", str(tmp_path)])
    train.release_engines()
    files = sorted(os.listdir(tmp_path / "caro"))
    assert files and all(f.startswith("best_") and f.endswith(".dat") for f in files)
    g = _caro(15, 5)
    for f in files:
        net = Net(g.obs_shape, g.action_space)
        net.load_state_dict(torch.load(str(tmp_path / "caro" / f), map_location="cpu"))
        for v in net.state_dict().values():
            assert torch.isfinite(v.float()).all()
    a, b = (str(tmp_path / "caro" / f) for f in (files[0], files[-1]))
    per_agent, per_pair = play.main(["-g", "2", "--cuda", a, b, "-r", "2"])
    assert sum(sum(v) for v in per_pair.values()) == 2 * 2
