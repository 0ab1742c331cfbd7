"""Virtual loss on the GPU (include/caro_hip.h, "virtual loss"; SelfPlayEngine.set_virtual_loss): every level of every
descent of step-wise games against the numpy rule (caro_ai_amd/virtual_loss.py) on the rows the engine holds, the counts
taken from the paths of the earlier descents as the engine reports them; the frozen rows and the real path records; the
launch forms against each other; off is off; the other extensions on top; the set call's errors; the train path.

Every engine here evaluates with the table net (HashNet).  The boards and shapes are those of
tests/test_gpu_forced_playouts.py; the helpers are those of that file and of tests/test_gpu_fpu.py."""
import numpy as np
import pytest

from caro_ai_amd import fpu
from caro_ai_amd import virtual_loss as vl
from tests.test_gpu_engine import DEV, _game_of
from tests.test_gpu_forced_playouts import (BOARDS, C4, C_PUCT, EXPLORE, FORMS, _Stepwise, _engine, _legal, _same,
                                            _shipped_net)
from tests.test_gpu_fpu import _lookup_keys, _Paths

pytestmark = pytest.mark.gpu

N_VL = 2
R, RR = 0.5, 0.25
ST_DROPPED = 0


def _check_paths(eng, game, paths, games, B, players, nz, n_vl, legal_cache, r=0.0, rr=0.0, fk=0.0, tally=None,
                 two_stores=False):
    """for b in order, every action on descent b's path is the rule's choice on the frozen row, the counts coming from the
    paths of descents 0 .. b-1 of the same game.  With `tally`, also counts the levels (root / below) where the rule with
    n_vl = 0 would have chosen otherwise."""
    items = [(g, b, i) for (g, b), (keys, acts) in sorted(paths.items()) for i in range(len(acts))]
    if not items:
        return
    keys = np.stack([paths[(g, b)][0][i] for g, b, i in items])
    rows = _lookup_keys(eng, [g for g, _, _ in items], [int(players[g]) if two_stores else 0 for g, _, _ in items], keys)
    assert rows["found"].all()
    at = {it: j for j, it in enumerate(items)}
    A = game.action_space
    for g in games:
        counts = {}
        for b in range(B):
            pkeys, acts = paths[(g, b)]
            q_up = np.float32(0.0)
            for i, a in enumerate(acts):
                j = at[(g, b, i)]
                kb = pkeys[i].tobytes()
                if kb not in legal_cache:
                    legal_cache[kb] = _legal(game, pkeys[i])
                root = i == 0
                N, W, Q, P, strong = (rows[x][j] for x in ("N", "W", "Q", "P", "strong"))
                c = np.array([counts.get((kb, x), 0) for x in range(A)], np.int64)
                args = (root, N, W, Q, P, strong, legal_cache[kb], nz[g, b] if root else None, C_PUCT, EXPLORE, c)
                rest = (q_up, rr if root else r, fk if root else 0.0)
                want = vl.level_choice(*args, n_vl, *rest)
                assert int(a) == want, (g, b, i, int(a), want, c.tolist())
                if tally is not None:
                    tally["levels"] += 1
                    if vl.level_choice(*args, 0, *rest) != want:
                        tally["root" if root else "below"] += 1
                q_up = fpu.raw_q_up(root, int(a), N, W, Q, strong)
            for i, a in enumerate(acts):  # (a board fixes its level: an edge appears once on a path)
                e = (pkeys[i].tobytes(), int(a))
                counts[e] = counts.get(e, 0) + 1


def _stepwise_levels(d, G, S, B, plies, sbt0, seed, evict=False, n_vl=N_VL, r=0.0, rr=0.0, fk=0.0, two_stores=False):
    """`plies` plies of G step-wise games; every minibatch selected twice from the same noise rows (n_vl = 0, cancelled;
    then n_vl) and every level of every descent of both selects checked against the numpy rule"""
    game = _game_of(d)
    kw = {"n_stores": 2} if two_stores else {}
    eng = _engine(game, G, S, B, sbt0, seed, evict=evict, **kw)
    if fk > 0.0:
        eng.set_forced_playouts(fk)
    if r > 0.0 or rr > 0.0:
        eng.set_fpu(r, rr)
    other = 1 if (fk > 0.0 or r > 0.0 or rr > 0.0 or two_stores) else 0
    sw = _Paths(eng, B)
    seen = dict(levels=0, root=0, below=0, stores=set())
    alive = np.ones(G, bool)
    legal_cache = {}
    kw = dict(r=r, rr=rr, fk=fk, two_stores=two_stores)
    for _ in range(plies):
        _, players, ply, uid = eng.roots()
        games = np.flatnonzero(alive).tolist()
        if not games:
            break
        seen["stores"].update(int(players[g]) for g in games)
        for mb in range(S):
            nz = sw.noise(uid, ply, mb)
            eng.set_virtual_loss(0)
            assert eng.kernel_form() == other
            sw.select(mb, nz)
            _check_paths(eng, game, sw.paths(games), games, B, players, nz, 0, legal_cache, **kw)
            sw.cancel()
            eng.set_virtual_loss(n_vl)
            assert eng.kernel_form() == 1
            sw.select(mb, nz)
            _check_paths(eng, game, sw.paths(games), games, B, players, nz, n_vl, legal_cache, tally=seen, **kw)
            sw.finish()
        _, done, _ = eng.step()
        alive &= done.cpu().numpy() == 0
    c = eng.counters()
    eng.close()
    assert c["overflows"] == 0
    return seen


@pytest.mark.parametrize("d,k,G,S,B,plies,sbt0,seed,evict", BOARDS,
                         ids=["-".join(str(v) for v in b[0].values()) for b in BOARDS])
def test_every_level_of_every_descent(d, k, G, S, B, plies, sbt0, seed, evict):
    """test 1"""
    seen = _stepwise_levels(d, G, S, B, plies, sbt0, seed, evict=evict)
    print("virtual loss, step-wise:", d, "levels checked", seen["levels"], "levels changed: root", seen["root"], "below",
          seen["below"])
    assert seen["root"] > 0, "the rule changed no root choice"
    if d == C4:
        assert seen["below"] > 0, "the rule changed no choice below the root"


def test_connect4_at_batch_8():
    """test 1, the shape of BOARDS' list that is one full wavefront per game through k_select"""
    seen = _stepwise_levels(C4, 8, 5, 8, 5, 4, 14)
    print("virtual loss, step-wise, C4 at B = 8: levels checked", seen["levels"], "levels changed: root", seen["root"],
          "below", seen["below"])
    assert seen["root"] > 0 and seen["below"] > 0


# ------------------------------------------------------------------ frozen rows, real path records
def _bits(x):
    return x.view(np.uint32) if x.dtype == np.float32 else x


def test_rows_stay_frozen_and_path_records_carry_real_counts():
    """test 2"""
    game = _game_of(C4)
    G, S, B = 8, 6, 8
    eng = _engine(game, G, S, B, 4, 9)
    eng.set_virtual_loss(N_VL)
    sw = _Paths(eng, B)
    games = list(range(G))
    shared = 0
    for ply_no in range(4):
        _, players, ply, uid = eng.roots()
        for mb in range(S):
            nz = sw.noise(uid, ply, mb)
            sw.select(mb, nz)
            paths = sw.paths(games)
            info = sw.info.cpu().numpy().reshape(G, B, 4)
            items = sorted({(g, keys[i].tobytes()) for (g, b), (keys, acts) in paths.items() for i in range(len(acts))})
            if not items:
                sw.finish()
                continue
            kk = np.stack([np.frombuffer(kb, np.uint64) for _, kb in items])
            gg = [g for g, _ in items]
            before = _lookup_keys(eng, gg, [0] * len(gg), kk)
            sw.cancel()
            after_cancel = _lookup_keys(eng, gg, [0] * len(gg), kk)
            for x in ("found", "N", "W", "Q", "P", "strong"):
                assert np.array_equal(_bits(before[x]), _bits(after_cancel[x])), x
            sw.select(mb, nz)
            again = sw.paths(games)
            for k2 in paths:  # (the same select from the same rows)
                assert np.array_equal(paths[k2][0], again[k2][0]) and np.array_equal(paths[k2][1], again[k2][1])
            during = _lookup_keys(eng, gg, [0] * len(gg), kk)
            for x in ("N", "W", "Q", "strong"):  # (caro_lookup_nodes after a select shows the frozen rows)
                assert np.array_equal(_bits(before[x]), _bits(during[x])), x
            sw.finish()
            after = _lookup_keys(eng, gg, [0] * len(gg), kk)
            want = np.zeros_like(before["N"])
            at = {it: j for j, it in enumerate(items)}
            for (g, b), (keys, acts) in paths.items():
                if info[g, b, 0] == ST_DROPPED:
                    continue
                for i, a in enumerate(acts):
                    want[at[(g, keys[i].tobytes())], int(a)] += 1
            assert np.array_equal(after["N"] - before["N"], want), (ply_no, mb)
            shared += int((want > 1).sum())
        eng.step()
    c = eng.counters()
    eng.close()
    assert c["overflows"] == 0 and shared > 0  # edges that several backed-up paths of one minibatch went through


# ------------------------------------------------------------------ whole games through every launch form
def _run(d, G, S, B, sbt0, seed, form, vl_calls=(), evict=False, forced=None, early=None, resign=None, cap=None,
         openings=None, fpu_pair=None, restart=False, forms_seen=None):
    """the games of uids 0 .. G-1 played to the end through one launch form -> ({uid: game}, counters)"""
    from caro_ai_amd.resign import split_games
    game = _game_of(d)
    eng = _engine(game, G, S, B, sbt0, seed, evict=evict, stagger=form == "stag", n_games=G)
    if resign is not None:
        eng.set_resign(*resign)
    if cap is not None:
        eng.set_playout_cap(*cap)
    if early is not None:
        eng.set_early_stop(early)
    if openings is not None:
        eng.set_openings(openings)
    if forced is not None:
        eng.set_forced_playouts(forced)
    if fpu_pair is not None:
        eng.set_fpu(*fpu_pair)
    if forms_seen is not None:
        forms_seen.append(eng.kernel_form())
    for n in vl_calls:
        eng.set_virtual_loss(n)
        if forms_seen is not None:
            forms_seen.append(eng.kernel_form())
    if restart:
        eng.restart()
        if forms_seen is not None:
            forms_seen.append(eng.kernel_form())
    hw = game.obs_shape[1] * game.obs_shape[2]
    games = {}
    for _ in range(hw + S + 8):
        if form == "stepwise":
            for mb in range(S):
                eng.minibatch(B, mb)
            eng.step()
        elif form == "move":
            eng.search_step(S, B)
        else:
            eng.search(S, B)
            eng.step()
        out = eng.drain(recycle=False)
        if out["games"].shape[0]:
            for g in split_games({kk: v.cpu().numpy().copy() for kk, v in out.items()}):
                assert g["uid"] not in games
                games[g["uid"]] = g
        if len(games) >= G:
            break
    c = eng.counters()
    eng.close()
    assert len(games) == G and c["overflows"] == 0
    return games, c


@pytest.mark.parametrize("d,G,S,B,sbt0,evict", FORMS, ids=["c4", "mnk-3-3", "mnk-8-4", "mnk-9-5", "mnk-15-5"])
def test_all_launch_forms_agree(d, G, S, B, sbt0, evict):
    """test 3: the step-wise kernels, the fused lock-step search, the one-call move and the staggered stream play the same
    games with the same tuples and the same counters; with one descent per minibatch they are the off engine's games"""
    ref, c0 = _run(d, G, S, B, sbt0, 31, "stepwise", [N_VL], evict=evict)
    off, c_off = _run(d, G, S, B, sbt0, 31, "fused", evict=evict)
    if B == 1:
        _same(off, ref, "one descent per minibatch: the off engine's games")
    else:
        assert any(not np.array_equal(ref[u]["states"], off[u]["states"]) for u in ref), "the feature changed no game"
    assert c_off["sims"] == c0["sims"] or B > 1
    for form in ("fused", "move", "stag"):
        got, c = _run(d, G, S, B, sbt0, 31, form, [N_VL], evict=evict)
        _same(ref, got, form)
        assert c["sims"] == c0["sims"] and c["plies"] == c0["plies"]


@pytest.mark.parametrize("form", ["stag", "fused"])
def test_off_is_off_and_restart_keeps_the_setting(form):
    """test 4"""
    never, c_never = _run(C4, 32, 5, 8, 6, 33, form)
    forms = []
    back, c_back = _run(C4, 32, 5, 8, 6, 33, form, [N_VL, 0], forms_seen=forms)
    assert forms == [0, 1, 0]
    _same(never, back, "0 after 2")
    assert c_never == c_back
    on, c_on = _run(C4, 32, 5, 8, 6, 33, form, [N_VL])
    forms = []
    again, c_again = _run(C4, 32, 5, 8, 6, 33, form, [N_VL], restart=True, forms_seen=forms)
    assert forms == [0, 1, 1]
    _same(on, again, "restarted")
    assert c_on == c_again
    assert any(not np.array_equal(on[u]["states"], never[u]["states"]) for u in on)


# ------------------------------------------------------------------ the other options on top
def test_levels_with_first_play_urgency_and_forced_playouts_on_top():
    """test 5, per level: a forced action (the test reading N' and nsum') wins the root level, an action with N' == 0 gets
    the substituted Q, every other choice follows the rule"""
    seen = _stepwise_levels(C4, 8, 6, 4, 6, 4, 4, r=R, rr=RR, fk=2.0)
    print("virtual loss with first-play urgency and forced playouts:", {x: seen[x] for x in ("levels", "root", "below")})
    assert seen["root"] > 0 and seen["below"] > 0


def test_levels_on_two_stores():
    """test 5, per level: an engine with two stores, each side's tree by the same rule"""
    seen = _stepwise_levels(C4, 4, 4, 8, 4, 0, 2, two_stores=True)
    print("virtual loss, two stores:", {x: seen[x] for x in ("levels", "root", "below")})
    assert seen["stores"] == {0, 1} and seen["root"] > 0


@pytest.mark.parametrize("d,G,S,B,sbt0,evict", [FORMS[0], FORMS[4]], ids=["c4", "mnk-15-5"])
def test_the_other_options_compose(d, G, S, B, sbt0, evict):
    """test 5, whole games: forced playouts, resignation, early stop, the playout cap and openings on top.  The forms that
    know a ply's budget -- the fused search, the one-call move, the staggered stream -- agree with all five on.  The
    step-wise loop is compared with the fused search without the cap and early stop (NOTES, "A narrowing in the
    composition test")."""
    kw = dict(evict=evict, forced=2.0, resign=(-0.2, 0.25), early=1, cap=(0.5, 2), openings=3)
    ref, c0 = _run(d, G, S, B, sbt0, 32, "fused", [N_VL], **kw)
    off, _ = _run(d, G, S, B, sbt0, 32, "fused", **kw)
    assert any(not np.array_equal(ref[u]["states"], off[u]["states"]) for u in ref), "the feature changed no game"
    for form in ("move", "stag"):
        got, c = _run(d, G, S, B, sbt0, 32, form, [N_VL], **kw)
        _same(ref, got, form)
        assert c["sims"] == c0["sims"] and c["plies"] == c0["plies"]
    kw["early"] = kw["cap"] = None
    ref, c0 = _run(d, G, S, B, sbt0, 32, "stepwise", [N_VL], **kw)
    got, c = _run(d, G, S, B, sbt0, 32, "fused", [N_VL], **kw)
    _same(ref, got, "fused, without early stop and the cap")
    assert c["sims"] == c0["sims"] and c["plies"] == c0["plies"]


# ------------------------------------------------------------------ errors, the training path
def test_set_call_errors():
    """test 6"""
    eng = _engine(_game_of(C4), 8, 4, 8, 4, 1)
    L = eng.L
    for bad in (-1, 17):
        assert L.caro_engine_set_virtual_loss(eng.h, bad) == -22
        with pytest.raises(ValueError):
            eng.set_virtual_loss(bad)
    assert eng.virtual_loss is None and eng.kernel_form() == 0
    sw = _Stepwise(eng, 8)
    sw.select(0, np.full((8, 8, 7), 1.0 / 7))
    assert L.caro_engine_set_virtual_loss(eng.h, N_VL) == -71  # a pending caro_select
    sw.cancel()
    eng.search(4, 8)
    eng.step()
    eng.drain_begin(False)
    assert L.caro_engine_set_virtual_loss(eng.h, N_VL) == -71  # a drain pending
    eng.drain_end()
    eng.set_virtual_loss(N_VL)
    assert eng.virtual_loss == N_VL and eng.kernel_form() == 1
    eng.set_virtual_loss(0)
    assert eng.virtual_loss == 0 and eng.kernel_form() == 0
    eng.close()


def test_self_play_with_virtual_loss_drops_fewer_descents():
    """test 6: tuples whose pi sums to 1, zero overflows (self_play raises on one), and fewer descents dropped as
    duplicates than the same run with the feature off"""
    from caro_ai_amd import train
    game = _game_of(C4)
    net = _shipped_net(game)
    buf = train.DeviceReplayBuffer(game, 1 << 14, DEV)
    off = train.self_play(game, buf, net, 32, device=DEV, seed=3, stagger=True, searches=6, batch=8)
    n = len(buf)
    on = train.self_play(game, buf, net, 32, device=DEV, seed=3, stagger=True, searches=6, batch=8, virtual_loss=N_VL)
    assert len(buf) > n + 32 and on["steps"] > 0
    pi = buf.pi[n:len(buf)].double().sum(1).cpu().numpy()
    assert np.allclose(pi, 1.0, atol=1e-6)
    print("dropped: off", off["dropped"], off["dropped_share"], "on", on["dropped"], on["dropped_share"])
    assert on["dropped"] < off["dropped"]
    out = train.self_play_stream(game, buf, net, 32, device=DEV, seed=3, searches=6, batch=8, virtual_loss=N_VL)
    assert out["steps"] > 0
    train.release_engines()
