"""The tree kernels' float32 arithmetic and backup order, checked with the fine grain of the table evaluator.

W of an edge is a float32 running sum, and the reference applies a minibatch's backups one after another, so the
contributions to one edge must be added in queue order (terminals by sim index, then new leaves first seen; expand_body
of csrc/caro_engine.hip holds three implementations of that rule).  The grain-0 table net cannot see the order: its
values are multiples of 2^-10, every sum of them is exact.  Grain 1 (include/caro_hip.h, "Table evaluator") has 24-bit
values, under which a sum added in another order rounds differently (tests/test_fine_table_net_cpu.py states how often).

(a) k_net_hash itself, both grains, every launch form, against the torch twin, bit for bit;
(b) whole games against the oracle at grain 1, one case per tree-kernel family and backup branch;
(c) root N / W / Q after searches from recorded positions, grain 1;
(d) which backup branch of expand_body ran, from the full form's diagnostic stamps -- the sequential fallback included;
(e) the order itself, under virtual loss, against a host-side running sum.

(b) .. (d) hold the kernels' float32 arithmetic (PUCT on 24-bit priors, W, Q = W / N) to the oracle's on values that use the
whole mantissa.  They do NOT see the order of a sum, and cannot: see the note above (e), which is the test that does."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.conftest import load_golden
from tests.test_gpu_engine import DEV, FORMS, _check_against_oracle, _game_of, _search_from_positions

pytestmark = pytest.mark.gpu

C4 = {"kind": "c4"}


@pytest.fixture(params=FORMS)
def form(request):
    """stepwise: the torch twin evaluates, the engine runs k_select / k_encode / k_expand_backup one by one; fused: the
    device table evaluator and the fused tree kernels (tests/test_gpu_engine.py)"""
    return request.param


# ------------------------------------------------------------------ (a) k_net_hash against the torch twin
def _planes(n, shape, seed):
    """n rows of planes: a third of the cells set, to 1 and to other non-zero values; -0.0 counts as not set"""
    rng = np.random.default_rng(seed)
    x = (rng.random((n,) + tuple(shape)) < 0.3) * rng.choice(np.array([1.0, 1.0, 0.5, -2.0], np.float32), (n,) + tuple(shape))
    x = x.astype(np.float32)
    x[rng.random(x.shape) < 0.05] *= np.float32(-1.0)  # some zeros become -0.0
    return np.ascontiguousarray(x)


def _outputs(rows, A):
    return (torch.full((rows, A), -1.0, dtype=torch.float32, device=DEV),
            torch.full((rows,), -9.0, dtype=torch.float32, device=DEV))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _same_rows(p, v, live, want_p, want_v, what):
    """the rows `live` (bool per output row) carry want_p / want_v (one row per live row, in row order) bit for bit,
    every other row still holds the sentinels"""
    torch.cuda.synchronize()
    p, v = p.cpu().numpy(), v.cpu().numpy()
    assert int(live.sum()) == len(want_v), what
    assert np.array_equal(p[live].view(np.uint32), want_p.view(np.uint32)), what
    assert np.array_equal(v[live].view(np.uint32), want_v.view(np.uint32)), what
    assert (p[~live] == -1.0).all() and (v[~live] == -9.0).all(), what


@pytest.mark.parametrize("grain", [0, 1])
@pytest.mark.parametrize("shape,A", [((2, 6, 7), 7), ((2, 3, 3), 9), ((2, 15, 15), 225)], ids=["c4", "t3", "g15"])
def test_table_kernel_equals_the_torch_twin_in_every_launch_form(shape, A, grain):
    """k_net_hash of csrc/caro_net.hip -- until now checked only through the engine -- on L = 1, 5, 64, 257 rows (15 x 15:
    450 planes and 225 actions per row, more than a wavefront's 64 lanes, so the lane loops run several trips), in the
    dense launch, the which = 1 launch, the two-net pair launch and the slot-row launches with one net and with two;
    outputs start as -1 / -9 and the rows outside a launch keep that."""
    from caro_ai_amd import _lib
    from caro_ai_amd.net_hip import HashNet
    from tests.synth_net import synth_numpy
    S0, S1 = 0x1111, (1 << 64) - 5
    n0, n1 = HashNet(shape, A, DEV, salt=S0, grain=grain), HashNet(shape, A, DEV, salt=S1, grain=grain)
    L_ = n0.L
    pool = _planes(600, shape, 1000 + A)
    ref = {s: synth_numpy(pool, A, s, grain) for s in (S0, S1)}  # computed once: row k of every launch is pool row k
    if grain:  # the exactness the definition promises (the twin's int64 -> float32 conversion loses nothing at 24 bits)
        for P, v in ref.values():
            mp, mv = P.astype(np.float64) * 2.0 ** 27, v.astype(np.float64) * 2.0 ** 24
            assert np.array_equal(mp, np.rint(mp)) and np.array_equal(mv, np.rint(mv))
            assert mp.min() >= 1 and mp.max() <= 2 ** 24 and np.abs(mv).max() <= 2 ** 24 - 1
    assert not np.array_equal(ref[S0][0], ref[S1][0])
    x = torch.from_numpy(pool).to(DEV)
    for L in (1, 5, 64, 257):
        # dense, which = 0: rows [0, L); max_rows beyond L launches idle wavefronts
        for spare in (0, 3):
            counts = torch.tensor([L, 7], dtype=torch.int32, device=DEV)
            p, v = _outputs(L + 9, A)
            _lib.check(L_.caro_net_forward(n0.h, x.data_ptr(), counts.data_ptr(), 0, L + spare, p.data_ptr(), v.data_ptr(),
                                           _stream()))
            live = np.arange(L + 9) < L
            _same_rows(p, v, live, ref[S0][0][:L], ref[S0][1][:L], ("dense", L, spare))
        # which = 1: rows [l0, l0 + L)
        l0 = 3
        counts = torch.tensor([l0, L], dtype=torch.int32, device=DEV)
        p, v = _outputs(l0 + L + 9, A)
        _lib.check(L_.caro_net_forward(n1.h, x.data_ptr(), counts.data_ptr(), 1, L, p.data_ptr(), v.data_ptr(), _stream()))
        live = (np.arange(l0 + L + 9) >= l0) & (np.arange(l0 + L + 9) < l0 + L)
        _same_rows(p, v, live, ref[S1][0][l0:l0 + L], ref[S1][1][l0:l0 + L], ("which 1", L))
        # pair: rows [0, L) through n0, [L, L + l1) through n1
        l1 = (L + 1) // 2
        counts = torch.tensor([L, l1], dtype=torch.int32, device=DEV)
        p, v = _outputs(L + l1 + 9, A)
        _lib.check(L_.caro_net_forward_pair(n0.h, n1.h, x.data_ptr(), counts.data_ptr(), L + l1, p.data_ptr(), v.data_ptr(),
                                            _stream()))
        live = np.arange(L + l1 + 9) < L + l1
        _same_rows(p, v, live, np.concatenate([ref[S0][0][:L], ref[S1][0][L:L + l1]]),
                   np.concatenate([ref[S0][1][:L], ref[S1][1][L:L + l1]]), ("pair", L))
        # slot rows: game g's j-th leaf at row g * B + j; games with no leaf, with B leaves and with some
        B = 8
        G = max(4, -(-L // 4))
        cnt = np.array([(0, B, 3, B, 0, 1, 5)[g % 7] for g in range(G)])
        rows = np.arange(G * B)
        live = (rows % B) < cnt[rows // B]
        for two in (False, True):
            cls = (np.arange(G) % 3 == 1).astype(np.int64) if two else np.zeros(G, np.int64)
            gp = torch.tensor((cnt | (cls << 8)).astype(np.int32), device=DEV)
            counts = torch.tensor([int(cnt[cls == 0].sum()), int(cnt[cls == 1].sum())], dtype=torch.int32, device=DEV)
            p, v = _outputs(G * B, A)
            _lib.check(L_.caro_net_forward_slots(n0.h, n1.h if two else None, x.data_ptr(), counts.data_ptr(), gp.data_ptr(),
                                                 G, B, p.data_ptr(), v.data_ptr(), _stream()))
            row_cls = cls[rows // B][live]
            wp = np.where(row_cls[:, None] == 1, ref[S1][0][:G * B][live], ref[S0][0][:G * B][live])
            wv = np.where(row_cls == 1, ref[S1][1][:G * B][live], ref[S0][1][:G * B][live])
            _same_rows(p, v, live, wp, wv, ("slots", L, two))
    # the two nets of a launch share one grain
    other = HashNet(shape, A, DEV, salt=S1, grain=1 - grain)
    counts = torch.tensor([1, 1], dtype=torch.int32, device=DEV)
    p, v = _outputs(4, A)
    assert L_.caro_net_forward_pair(n0.h, other.h, x.data_ptr(), counts.data_ptr(), 2, p.data_ptr(), v.data_ptr(),
                                    _stream()) == -22  # CARO_E_INVAL
    _same_rows(p, v, np.zeros(4, bool), ref[S0][0][:0], ref[S0][1][:0], "refused pair")
    for n in (n0, n1, other):
        n.close()


def test_table_net_grain_is_0_or_1():
    from caro_ai_amd import _lib
    from caro_ai_amd.net_hip import HashNet
    with pytest.raises(_lib.CaroError, match="grain must be 0 or 1"):
        HashNet((2, 6, 7), 7, DEV, grain=2)


# ------------------------------------------------------------------ (b) whole games against the oracle, grain 1
def _lanes_per_descent(A):
    return 8 if A == 7 else 16 if A <= 16 else 32 if A <= 32 else 64


def _tree_kernel(game, B, form, stagger):
    """the kernel family a search of this geometry runs (include/caro_hip.h, caro_search_batch / caro_search_staggered)"""
    if form == "stepwise":
        return "k_select + k_expand_backup"
    t = B * _lanes_per_descent(game.action_space)
    if t == 64:
        return "k_tree_stag" if stagger else "k_tree"
    if t > 64 and t % 64 == 0:
        return "k_tree_stag_mw" if stagger else "k_tree_mw"
    return "k_select + k_expand_backup"


def _mnk(n, k):
    return {"kind": "mnk", "n": n, "k": k}


# id: (game, G, n_finish, sbt0, S, B, stores, salts, engine keywords, fused only, fused kernel, fused kernel form)
GAMES = {
    "c4-lean-one-wave": (C4, 16, 24, 4, 12, 8, 1, None, {}, False, "k_tree", 0),
    "c4-full-two-nets": (C4, 16, 16, 0, 12, 8, 2, (0x1111, 0x2222), {}, False, "k_tree", 1),
    "c4-multi-wave": (C4, 8, 8, 4, 10, 16, 1, None, {}, False, "k_tree_mw", None),
    "c4-general-owner-loop": (C4, 4, 4, 2, 8, 64, 1, None, {}, False, "k_tree_mw", None),
    "c4-staggered": (C4, 16, 24, 4, 12, 8, 1, None, dict(stagger=True, searches_hint=12), True, "k_tree_stag", 0),
    "c4-staggered-multi-wave-evict": (C4, 8, 12, 4, 10, 16, 1, None, dict(stagger=True, evict=True, searches_hint=10), True,
                                      "k_tree_stag_mw", None),
    "t3-16-lanes-draws": (_mnk(3, 3), 32, 64, 2, 6, 4, 1, None, {}, False, "k_tree", 0),
    "m4-16x4": (_mnk(4, 3), 8, 12, 2, 6, 4, 1, None, {}, False, "k_tree", 0),
    "m5-32x2": (_mnk(5, 4), 8, 12, 2, 12, 2, 1, None, {}, False, "k_tree", 0),
    "m8-64x1": (_mnk(8, 5), 8, 8, 2, 10, 1, 1, None, {}, False, "k_tree", 0),
    "m10-2-per-lane": (_mnk(10, 5), 4, 4, 3, 6, 8, 1, None, {}, False, "k_tree_mw", None),
    "m15-4-per-lane": (_mnk(15, 5), 4, 4, 3, 5, 8, 1, None, {}, False, "k_tree_mw", None),
    "caro9-evict": ({"kind": "caro", "n": 9, "k": 5}, 4, 4, 3, 6, 8, 1, None, dict(evict=True), False, "k_tree_mw", None),
}


# the staggered schedule needs the device-side evaluator: those cases exist in the fused form only
GAME_RUNS = [(case, f) for case in GAMES for f in FORMS if f == "fused" or not GAMES[case][9]]


@pytest.mark.parametrize("case,form", GAME_RUNS, ids=["%s-%s" % cf for cf in GAME_RUNS])
def test_games_equal_the_oracle_with_fine_values(case, form):
    """every game of the run equals the oracle's game of the same uid (states, pi bit for bit, z, result) with 24-bit
    priors and values: one case per tree-kernel family, lane geometry and backup branch of expand_body.  The kernel the
    fused form runs is stated per case and checked against the geometry; for the one-wave kernels so is the compiled
    form (0 lean, 1 full)."""
    d, G, n_finish, sbt0, S, B, stores, salts, kw, fused_only, kernel, kform = GAMES[case]
    assert form == "fused" or not fused_only
    game = _game_of(d)
    ran = _tree_kernel(game, B, form, kw.get("stagger", False))
    seen = {}

    def look(eng):
        seen["form"] = eng.kernel_form()

    c, ref, games = _check_against_oracle(d, G, n_finish, sbt0, S, B, stores, seed=900 + len(case), uid_base=100, form=form,
                                          salts=salts, grain=1, on_engine=look, **kw)
    print("%s / %s: %s, kernel form %d, %d games, %d sims" % (case, form, ran, seen["form"], len(games), c["sims"]))
    if form == "fused":
        assert ran == kernel
        if kform is not None:
            assert seen["form"] == kform
    assert len(games) >= n_finish
    if case == "t3-16-lanes-draws":
        assert (games[:, 2] == 0).any(), "no drawn game in the sample"


# ------------------------------------------------------------------ (c) W itself, from recorded positions
def test_root_sums_from_recorded_connect4_positions_with_fine_values(form):
    """the first 300 unfinished recorded connect-four positions, 6 x 8 sims on an empty tree: root N, W (the float32
    running sum, several same-minibatch contributions per root edge), strong flags, Q, tree size and pi equal the
    oracle's"""
    d = load_golden("rules_c4.json.gz")
    recs = [r for r in d["recs"] if not r["won"]][:300]
    counts = []
    checked, with_terminals = _search_from_positions(C4, recs, 6, 8, seed=151, form=form, root_counts=counts, grain=1)
    assert checked >= 280
    # the sums under test exist: most roots have an edge that was visited more than twice
    assert (np.stack(counts).max(1) > 2).mean() > 0.9


def test_root_sums_from_recorded_tictactoe_positions_with_fine_values(form):
    """200 unfinished recorded 3 x 3 positions, 8 x 4 sims: the same comparison (terminal values +-1 and 0 among the
    24-bit ones)"""
    d = load_golden("rules_ttt3.json.gz")
    recs = [r for r in d["recs"] if not r["won"]][:200]
    checked, with_terminals = _search_from_positions(_mnk(3, 3), recs, 8, 4, seed=152, form=form, grain=1)
    assert checked >= 150 and with_terminals > 50


# ------------------------------------------------------------------ (d) which backup branch ran
def _stamp_totals(eng, into):
    """switch the diagnostic stamps on (the one-wave kernels then run their full form) and collect, after every search
    call, slot 7 of each game's expand_body stamps: the entry count `total` of the game's last backup"""
    from caro_ai_amd import _lib
    _lib.check(eng.L.caro_debug_stamps(eng.h, 1))
    G = eng.G
    search = eng.search

    def search_and_read(*a, **k):
        r = search(*a, **k)
        torch.cuda.synchronize()
        out = np.zeros(G * 16, np.uint64)
        _lib.check(eng.L.caro_debug_read(eng.h, out.ctypes.data, out.size, None))
        into.extend(out.reshape(2, G, 8)[1, :, 7].astype(np.int64).tolist())
        return r

    eng.search = search_and_read


@pytest.mark.parametrize("case", ["c4-lean-one-wave", "c4-general-owner-loop"])
def test_the_backup_branch_that_ran(case, form):
    """expand_body applies the owners' sums in one of three ways: the one-wave ballot form (2 .. 128 entries in a
    minibatch's queue), the general owner loop (more than 128) and the sequential fallback (more than MAXE = 512 / 256).
    With the diagnostic stamps on, the 12 x 8 games must have run the first and the 8 x 64 games the second -- and still
    equal the oracle's, stamps or not.  (Seen: 2 .. 25 entries in the 12 x 8 games, up to 192 in the 8 x 64 games; the
    third way is test_the_sequential_fallback_runs_from_late_positions.)"""
    d, G, n_finish, sbt0, S, B, stores, salts, kw, _, _, _ = GAMES[case]
    totals = []
    _check_against_oracle(d, G, n_finish, sbt0, S, B, stores, seed=900 + len(case), uid_base=100, form=form, salts=salts,
                          grain=1, on_engine=lambda eng: _stamp_totals(eng, totals), **kw)
    totals = np.array(totals)
    assert len(totals) >= G
    print("%s / %s: entries per backup (last minibatch of every move): min %d, max %d, over 128: %d of %d"
          % (case, form, totals.min(), totals.max(), int((totals > 128).sum()), len(totals)))
    if case == "c4-lean-one-wave":
        assert totals.max() <= 128 and ((totals >= 2) & (totals <= 128)).any()
    else:
        assert (totals > 128).any() and totals.max() <= 512


def test_the_sequential_fallback_runs_from_late_positions(form):
    """more than MAXE = 512 entries in one backup: 64 descents that all end deeper than 8 plies below the root.  Whole
    games do not get there; a long search from a late position does, once its principal line reaches a terminal 9 or
    more plies down and all 64 descents of a minibatch walk it (13 .. 15 empty cells, 192 x 64 sims).  The recorded
    unfinished connect-four positions with 10 .. 20 empty cells, one engine slot each: the stamps of the closing
    minibatch show the slots that took the fallback, and those slots (and four others) equal the oracle's search --
    root N, W, Q, strong flags, tree size, pi."""
    from oracle.oracle import Oracle
    d = load_golden("rules_c4.json.gz")
    o, game = Oracle(Oracle.C4), _game_of(C4)
    recs = [r for r in d["recs"] if not r["won"]]
    recs = [r for r in recs if 10 <= int((o.to_cells(int(r["s2"])) == 0).sum()) <= 20
            and game.possible_moves(int(r["s2"]))][:384]
    totals = []

    def slots():
        over = np.flatnonzero(np.array(totals) > 512).tolist()
        print("sequential fallback / %s: entries of the closing backup: max %d, over 128: %d, over 512: slots %r"
              % (form, max(totals), int((np.array(totals) > 128).sum()), [(g, totals[g]) for g in over]))
        assert over, "no slot's closing backup had more than 512 entries"
        return sorted(set(over) | {0, 1, 2, 3})

    checked, _ = _search_from_positions(C4, recs, 192, 64, seed=77, form=form, grain=1,
                                        on_engine=lambda eng: _stamp_totals(eng, totals), only=slots)
    assert len(totals) == len(recs) and checked >= 5


# ------------------------------------------------------------------ (e) where the order can show: virtual loss
# In the plain search the descents of one minibatch differ in their root noise only: two of them that go through the
# same edge walk the same frozen tree below it and end in the same place, so an edge's entries of one minibatch are one
# new leaf (its duplicates are dropped) or several visits of ONE terminal -- equal values, whose sum has no order.  (A
# build whose owner loops add an edge's entries in descending index passes (b), (c) and (d) for that reason; measured.)
# With virtual loss (caro_engine_set_virtual_loss) the later descents of a minibatch are pushed off the earlier ones'
# paths BELOW shared edges: then an edge receives different leaves' values in one minibatch and the queue order decides W.
def _vl_engine(game, G, S, B, seed, grain=1, n_vl=2):
    from caro_ai_amd.engine import SelfPlayEngine
    from caro_ai_amd.net_hip import HashNet
    hw = game.obs_shape[1] * game.obs_shape[2]
    eng = SelfPlayEngine(game, G, evaluators=[HashNet(game, device=DEV, grain=grain)], max_batch=B, steps_before_tau_0=4,
                         seed=seed, device=DEV, searches_hint=S, node_cap=S * B * hw + 64)
    eng.set_virtual_loss(n_vl)
    return eng


def _f32(x):
    return np.float32(x)


@pytest.mark.parametrize("G,S,B,plies", [(8, 6, 8, 4), (2, 4, 64, 3)], ids=["one-wave-owners", "general-owner-loop"])
def test_backup_sums_keep_queue_order_under_virtual_loss(G, S, B, plies):
    """step-wise connect four with virtual loss 2 and the 24-bit table net: after every minibatch, W of every edge on a
    backed-up path is the float32 running sum of mcts.py:225-246 applied item by item in the reference's queue order --
    terminals by sim index, then new leaves first seen, each from the leaf upwards with the sign flipping per ply --
    starting from the edge's W before the minibatch; N and Q = W / N likewise.  The leaf values are the rows the table
    kernel returned (checked against its twin in (a)), matched to the descents by leaf key.  The test states its own
    sensitivity: it counts the edges whose sum would come out differently in the reversed order, and needs some."""
    from tests.test_gpu_fpu import _Paths, _lookup_keys
    game = _game_of(C4)
    eng = _vl_engine(game, G, S, B, seed=9)
    sw = _Paths(eng, B)
    games = list(range(G))
    shared = order_matters = max_entries = 0
    for ply_no in range(plies):
        _, players, ply, uid = eng.roots()
        for mb in range(S):
            sw.select(mb, sw.noise(uid, ply, mb))
            paths = sw.paths(games)
            info = sw.info.cpu().numpy().reshape(G, B, 4)
            tval = sw.value.cpu().numpy().reshape(G, B)
            leaf = sw.leaf.cpu().numpy().view(np.uint64).reshape(G, B, -1)
            items = sorted({(g, keys[i].tobytes()) for (g, b), (keys, acts) in paths.items() for i in range(len(acts))})
            if not items:  # an unexpanded root: the minibatch only expands it, nothing is backed up
                sw.finish()
                continue
            at = {it: j for j, it in enumerate(items)}
            kk = np.stack([np.frombuffer(kb, np.uint64) for _, kb in items])
            gg = [g for g, _ in items]
            before = _lookup_keys(eng, gg, [0] * len(gg), kk)
            sw.finish()
            torch.cuda.synchronize()
            after = _lookup_keys(eng, gg, [0] * len(gg), kk)
            row_keys = eng.leaf_keys.cpu().numpy().view(np.uint64)
            row_val = eng._values.cpu().numpy()
            W = before["W"].copy()
            N = before["N"].copy()
            lists = {}
            row = 0
            for g in games:  # dense rows: game by game, a game's new leaves in first-seen order
                queue = [(b, _f32(tval[g, b])) for b in range(B) if info[g, b, 0] == 1]
                for b in range(B):
                    if info[g, b, 0] == 2:
                        assert np.array_equal(row_keys[row], leaf[g, b]), (g, b, row)
                        queue.append((b, _f32(row_val[row])))
                        row += 1
                max_entries = max(max_entries, sum(len(paths[(g, b)][1]) for b, _ in queue))
                for b, v in queue:
                    keys, acts = paths[(g, b)]
                    n = len(acts)
                    for i in range(n - 1, -1, -1):
                        e = (at[(g, keys[i].tobytes())], int(acts[i]))
                        c = v if (n - 1 - i) & 1 else -v
                        W[e] = _f32(W[e] + c)
                        N[e] += 1
                        lists.setdefault(e, []).append(c)
            for e, cs in lists.items():
                if len(cs) > 1:
                    shared += 1
                    w = before["W"][e]
                    for c in reversed(cs):
                        w = _f32(w + c)
                    order_matters += int(w != W[e])
            assert np.array_equal(after["N"], N), (ply_no, mb)
            assert np.array_equal(after["W"].view(np.uint32), W.view(np.uint32)), (ply_no, mb)
            for e in lists:
                assert after["Q"][e] == _f32(W[e] / _f32(N[e])), (ply_no, mb, e)
        eng.step()
    c = eng.counters()
    eng.close()
    print("virtual loss, B = %d: edges with several entries in a minibatch %d, of which the reversed order changes W: %d; "
          "most entries in one backup %d" % (B, shared, order_matters, max_entries))
    assert c["overflows"] == 0
    assert order_matters > 0
    assert max_entries > 128 if B == 64 else 2 <= max_entries <= 128


@pytest.mark.parametrize("G,S,B,moves", [(8, 6, 8, 6), (2, 4, 64, 4)], ids=["k_tree", "k_tree_mw"])
def test_fused_search_equals_step_wise_search_under_virtual_loss(G, S, B, moves):
    """the fused tree kernels against the step-wise ones (which the test above holds to the reference's order): virtual
    loss 2, the 24-bit table net, the same seed -- after every move's search the root rows (N, W, Q) of all games are
    the same bits, through caro_search_batch + caro_step and through caro_search_move"""
    game = _game_of(C4)
    engs = [_vl_engine(game, G, S, B, seed=12) for _ in range(3)]
    for _ in range(moves):
        rows = []
        for k, eng in enumerate(engs):
            keys = eng.roots()[0]
            states = [game.from_key(x) for x in keys]
            if k == 0:
                for mb in range(S):
                    eng.minibatch(B, mb)
            elif k == 1:
                eng.search(S, B)
            if k < 2:
                rows.append(eng.lookup(list(range(G)), [0] * G, states))
                eng.step()
            else:
                eng.search_step(S, B)
        assert rows[0]["found"].all() and rows[0]["N"].sum() > 0
        for x in ("found", "N", "W", "Q", "P", "strong"):
            a, b = rows[0][x], rows[1][x]
            assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                  b.view(np.uint32) if b.dtype == np.float32 else b), x
        k0, k2 = engs[0].roots()[0], engs[2].roots()[0]
        assert np.array_equal(np.asarray(k0), np.asarray(k2))  # the one-call form made the same moves
    for eng in engs:
        assert eng.counters()["overflows"] == 0
        eng.close()
