"""Forced playouts and policy target pruning on the GPU (include/caro_hip.h, "forced playouts";
SelfPlayEngine.set_forced_playouts): every root choice of step-wise games against the numpy rule
(caro_ai_amd/forced_playouts.py) on the root row the engine holds; every drained tuple's pi against the pruned row; the
launch forms against each other; the other extensions on top of it; off is off; the train CLI.

Every engine here evaluates with the table net (HashNet).  Step-wise games are those of uids 0 .. G-1, first player =
uid & 1.  They are ended by resignation once the plies under test are made (threshold 1: every mover resigns), so a drain
hands out their tuples without the boards being played to the end."""
import ctypes as C

import numpy as np
import pytest
import torch

from caro_ai_amd import forced_playouts as fp
from oracle.oracle import sample_index
from tests.openings_ref import host_opening
from tests.test_gpu_engine import DEV, _game_of

pytestmark = pytest.mark.gpu

C4 = {"kind": "c4"}
EXPLORE, ALPHA, C_PUCT = 0.25, 0.3, 1.0


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _engine(game, G, S, B, sbt0, seed, evict=False, stagger=False, n_games=0, **kw):
    from caro_ai_amd.engine import SelfPlayEngine
    from caro_ai_amd.net_hip import HashNet
    hw = game.obs_shape[1] * game.obs_shape[2]
    return SelfPlayEngine(game, G, evaluators=[HashNet(game, device=DEV)], max_batch=B, steps_before_tau_0=sbt0,
                          seed=seed, device=DEV, searches_hint=S, stagger=stagger, stagger_recycle=False,
                          games_limit=n_games, evict=evict, node_cap=S * B * hw + 64, c_puct=C_PUCT, alpha=ALPHA,
                          explore=EXPLORE, **kw)


class _Stepwise:
    """the step-wise C-ABI around one engine: caro_select with explicit noise rows, every descent's first action"""

    def __init__(self, eng, B):
        self.eng, self.B, self.L = eng, B, eng.L
        G, dev = eng.G, eng.device
        self.info = torch.zeros((G * B, 4), dtype=torch.int32, device=dev)
        self.value = torch.zeros(G * B, dtype=torch.float32, device=dev)
        self.leaf = torch.zeros((G * B, eng.KW), dtype=torch.int64, device=dev)
        self.pkeys = torch.zeros((eng.HW, eng.KW), dtype=torch.int64, device=dev)  # (the states list: not compared)
        self.pact = torch.zeros((G * B, eng.HW), dtype=torch.int32, device=dev)

    def noise(self, uids, plies, mb):
        eng, B = self.eng, self.B
        nz = np.zeros((eng.G, B, eng.A))
        row = (C.c_double * eng.A)()
        for g in range(eng.G):
            for b in range(B):
                assert self.L.caro_host_noise_row(eng.cfg.seed, int(uids[g]), int(plies[g]), mb * B + b, eng.A, ALPHA,
                                                  row) == 0
                nz[g, b] = row[:]
        return nz

    def select(self, mb, nz):
        from caro_ai_amd import _lib
        eng = self.eng
        self.nz = torch.as_tensor(nz).to(eng.device).contiguous()
        _lib.check(self.L.caro_select(eng.h, self.B, mb, _ptr(self.nz), _ptr(eng.planes), _ptr(eng.leaf_keys),
                                      eng._stream()))

    def first_actions(self, games):
        """(path length, first action) of every descent of `games` in the pending select: int arrays [G, B]"""
        from caro_ai_amd import _lib
        eng, B = self.eng, self.B
        for g in games:
            for b in range(B):
                i = g * B + b
                _lib.check(self.L.caro_get_descent(eng.h, g, b, _ptr(self.info[i]), _ptr(self.value[i:i + 1]),
                                                   _ptr(self.leaf[i]), _ptr(self.pkeys), _ptr(self.pact[i]),
                                                   eng._stream()))
        info = self.info.cpu().numpy().reshape(eng.G, B, 4)
        return info[:, :, 1].copy(), self.pact.cpu().numpy().reshape(eng.G, B, -1)[:, :, 0].copy()

    def cancel(self):
        from caro_ai_amd import _lib
        _lib.check(self.L.caro_select_cancel(self.eng.h))

    def finish(self):
        """the net and expand + backup of the pending select, as SelfPlayEngine.minibatch does"""
        from caro_ai_amd import _lib
        eng, st = self.eng, self.eng._stream()
        eng.evaluators[0].forward_dev(eng.planes, eng._counts_dev, 0, eng.G * self.B, eng._probs, eng._values, st)
        _lib.check(self.L.caro_expand_backup(eng.h, _ptr(eng._probs), _ptr(eng._values), st))


def _legal(game, key):
    from caro_ai_amd import _lib
    from tests.openings_ref import kind_of
    kind, n, k = kind_of(game)
    out = (C.c_uint8 * game.action_space)()
    kk = (C.c_uint64 * 8)(*[int(x) for x in key])
    assert _lib.load().caro_host_legal(kind, n, k, kk, out) == 0
    return np.array(out[:], bool)


def _stepwise_games(d, k, G, S, B, plies, sbt0, seed, evict=False, cap=None, resign=None, early=None):
    """Tests 1 and 2 (and the step-wise halves of test 4) on one board: `plies` plies of G games, every minibatch selected
    twice from the same noise rows (k = 0, cancelled; then k), every root choice and every ply checked against the numpy
    rule; then every game resigns and the drained tuples are checked.  Returns the tallies of what was seen."""
    from caro_ai_amd import _lib
    from caro_ai_amd.resign import split_games
    L = _lib.load()
    game = _game_of(d)
    A = game.action_space
    eng = _engine(game, G, S, B, sbt0, seed, evict=evict)
    resign = resign or (-1.0, 0.0)  # (recording alone: Q >= -1 never resigns)
    eng.set_resign(*resign)
    if cap is not None:
        eng.set_playout_cap(*cap)
    if early is not None:
        eng.set_early_stop(early)
    sw = _Stepwise(eng, B)
    seen = dict(root=0, forced=0, moved=0, pruned_plies=0, removed=0, fast_plies=0, fast_descents=0, tau0=0, resigned=0)
    want = {g: [] for g in range(G)}  # per game and ply: (pi of the tuple, action, root q, minibatches)
    alive = np.ones(G, bool)
    for ply_no in range(plies + 1):
        if ply_no == plies:  # the closing ply: every mover resigns (q < 1; a q of exactly 1 plays its winning move)
            eng.set_resign(1.0, 0.0)
            resign = (1.0, 0.0)
        keys, players, ply, uid = eng.roots()
        states = game.from_keys(keys)
        games = np.flatnonzero(alive).tolist()
        legal = {g: _legal(game, keys[g]) for g in games}
        fast = {g: cap is not None and not L.caro_host_cap_uniform(seed, int(uid[g]), int(ply[g])) < cap[0] for g in games}
        for mb in range(S):
            sel = [g for g in games if not (fast[g] and mb >= cap[1])]  # (a fast ply selects nothing from `fast` on)
            row = eng.lookup(list(range(G)), [0] * G, states)
            nz = sw.noise(uid, ply, mb)
            eng.set_forced_playouts(0.0)
            sw.select(mb, nz)
            len_off, act_off = sw.first_actions(sel)
            sw.cancel()
            eng.set_forced_playouts(k)
            before = fp.stats(eng)
            sw.select(mb, nz)
            len_on, act_on = sw.first_actions(sel)
            root = forced = 0
            for g in sel:
                if not row["found"][g]:  # an unexpanded root: every descent ends at it
                    assert (len_off[g] == 0).all() and (len_on[g] == 0).all()
                    continue
                for b in range(B):
                    f = fp.forced_root(row["N"][g], row["P"][g], nz[g, b], legal[g], EXPLORE, 0.0 if fast[g] else k)
                    exp = int(np.argmax(f)) if f.any() else int(act_off[g, b])
                    assert len_on[g, b] >= 1 and act_on[g, b] == exp, (d, ply_no, mb, g, b, f.tolist())
                    if fast[g]:
                        seen["fast_descents"] += 1
                        assert act_on[g, b] == act_off[g, b]
                    else:
                        root += 1
                        forced += bool(f.any())
                        seen["moved"] += bool(f.any() and exp != act_off[g, b])
            after = fp.stats(eng)
            assert after["root_descents"] - before["root_descents"] == root
            assert after["forced_descents"] - before["forced_descents"] == forced
            seen["root"] += root
            seen["forced"] += forced
            sw.finish()
        # the ply: N' and pi' from the root row, the move from the unpruned pi
        row = eng.lookup(list(range(G)), [0] * G, states)
        before = fp.stats(eng)
        exp_act = {}
        pruned = removed = 0
        for g in games:
            N = row["N"][g].astype(np.int64)
            assert N.sum() > 0
            b = int(np.argmax(N))
            q = fp.edge_q(row["N"][g], row["W"][g], row["Q"][g], row["strong"][g])
            tau1 = sbt0 > 0 and ply[g] < sbt0  # (no openings here: step == ply)
            pi = N / np.float64(N.sum()) if tau1 else np.eye(A)[b]
            pi_t = pi
            if tau1 and not fast[g]:
                n2, b2 = fp.prune(N, q, row["P"][g], C_PUCT, k)
                assert b2 == b
                pi_t = n2.astype(np.float64) / np.float64(int(n2.sum()))
                pruned += int(n2.sum() < N.sum())
                removed += int(N.sum() - n2.sum())
            seen["tau0"] += not tau1
            seen["fast_plies"] += bool(fast[g])
            gives_up = q[b] < resign[0] and not L.caro_host_resign_uniform(seed, int(uid[g])) < resign[1]
            a = _lib.RESIGNED if gives_up else sample_index(pi, L.caro_host_move_uniform(seed, int(uid[g]), int(ply[g])))
            exp_act[g] = a
            want[g].append((pi_t, a, q[b], S if not fast[g] else min(S, cap[1])))
        actions, done, _ = eng.step()
        actions, done = actions.cpu().numpy(), done.cpu().numpy()
        after = fp.stats(eng)
        assert after["pruned_plies"] - before["pruned_plies"] == pruned
        assert after["visits_removed"] - before["visits_removed"] == removed
        seen["pruned_plies"] += pruned
        seen["removed"] += removed
        for g in games:
            assert actions[g] == exp_act[g], (d, ply_no, g)
            seen["resigned"] += actions[g] == _lib.RESIGNED
        alive &= done == 0
    out = eng.drain(recycle=False)
    c = eng.counters()
    eng.close()
    assert c["overflows"] == 0
    checked = 0
    for gm in split_games({kk: v.cpu().numpy() for kk, v in out.items()}):
        w = want[gm["uid"]]
        assert len(gm["pi"]) == len(w)
        for i, (pi_t, a, q, mbs) in enumerate(w):
            assert np.array_equal(gm["pi"][i].view(np.uint64), pi_t.view(np.uint64)), (d, gm["uid"], i)  # bit for bit
            assert gm["q"][i] == q
            if "mb" in gm:
                assert gm["mb"][i] == mbs
            if not (sbt0 > 0 and i < sbt0):
                assert sorted(gm["pi"][i].tolist())[-2:] == [0.0, 1.0]  # a tau = 0 ply stays one-hot
            checked += 1
    seen["tuples"] = checked
    return seen


BOARDS = [  # d, k, G, S, B, plies, sbt0, seed, evict
    ({"kind": "mnk", "n": 3, "k": 3}, 2.0, 8, 6, 4, 4, 3, 3, False),
    (C4, 2.0, 8, 6, 4, 6, 4, 4, False),
    ({"kind": "mnk", "n": 8, "k": 4}, 2.0, 8, 6, 4, 5, 4, 5, False),      # A = 64: one action per lane, 64 lanes
    ({"kind": "mnk", "n": 9, "k": 5}, 2.0, 8, 6, 4, 5, 4, 6, False),      # A = 81: two actions per lane
    ({"kind": "mnk", "n": 15, "k": 5}, 2.0, 4, 4, 8, 4, 3, 7, True),      # the multi-wave kernels, with eviction
    ({"kind": "caro", "n": 4, "k": 3}, 2.0, 8, 6, 4, 5, 4, 8, False),
]


@pytest.mark.parametrize("d,k,G,S,B,plies,sbt0,seed,evict", BOARDS,
                         ids=["-".join(str(v) for v in b[0].values()) for b in BOARDS])
def test_every_root_choice_and_every_pruned_tuple(d, k, G, S, B, plies, sbt0, seed, evict):
    """tests 1 and 2"""
    seen = _stepwise_games(d, k, G, S, B, plies, sbt0, seed, evict=evict)
    print("forced playouts, step-wise:", d, "k", k, seen)
    assert seen["root"] > 0 and seen["moved"] >= 1, "no descent was forced away from the usual choice"
    assert seen["pruned_plies"] >= 1 and seen["removed"] >= 1, "no ply lost a visit to pruning"
    assert seen["tau0"] >= 1 and seen["tuples"] >= G


def test_fast_plies_are_neither_forced_nor_pruned():
    """test 4, playout cap (0.5, 2): per ply through the step-wise differential"""
    seen = _stepwise_games(C4, 2.0, 8, 6, 4, 6, 4, 4, cap=(0.5, 2))
    print("forced playouts with the playout cap:", seen)
    assert seen["fast_plies"] >= 4 and seen["fast_descents"] >= 16 and seen["moved"] >= 1 and seen["pruned_plies"] >= 1


def test_resignation_and_early_stop_read_the_unpruned_row():
    """test 4, step-wise half: with resignation (threshold -0.2, a quarter of the games playing through) and early stop
    on, every move, the recorded minibatches and the root Q are those of the unpruned counts"""
    seen = _stepwise_games(C4, 2.0, 16, 6, 4, 8, 6, 4, resign=(-0.2, 0.25), early=1)
    print("forced playouts with resignation and early stop:", seen)
    assert seen["moved"] >= 1 and seen["pruned_plies"] >= 1 and seen["tuples"] >= 16


# ------------------------------------------------------------------ whole games through every launch form
def _run(d, G, S, B, sbt0, seed, form, k=None, evict=False, early=None, resign=None, cap=None, openings=None,
         n_games=None, restart=False):
    """the games of uids 0 .. n_games-1 played to the end through one launch form -> ({uid: game}, stats, counters)"""
    from caro_ai_amd.resign import split_games
    game = _game_of(d)
    n_games = n_games or G
    eng = _engine(game, G, S, B, sbt0, seed, evict=evict, stagger=form == "stag", n_games=n_games)
    if resign is not None:
        eng.set_resign(*resign)
    if cap is not None:
        eng.set_playout_cap(*cap)
    if early is not None:
        eng.set_early_stop(early)
    if openings is not None:
        eng.set_openings(openings)
    if k is not None:
        for kk in (k if isinstance(k, (list, tuple)) else [k]):
            eng.set_forced_playouts(kk)
    if restart:
        eng.restart()
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
        if len(games) >= n_games:
            break
    st, c = fp.stats(eng), eng.counters()
    eng.close()
    assert len(games) == n_games and c["overflows"] == 0
    return games, st, c


def _same(a, b, what):
    assert sorted(a) == sorted(b), what
    for uid in a:
        for key in ("states", "players", "pi", "z", "mb", "full", "q", "open"):
            if key in a[uid] and a[uid][key] is not None:
                np.testing.assert_array_equal(a[uid][key], b[uid][key], err_msg="%s: %s of uid %d" % (what, key, uid))
        assert [a[uid][x] for x in ("first", "result", "steps")] == [b[uid][x] for x in ("first", "result", "steps")]


FORMS = [  # d, G, S, B, sbt0, evict
    (C4, 64, 5, 8, 6, False),                                 # one wavefront per game: k_tree, k_tree_stag
    ({"kind": "mnk", "n": 3, "k": 3}, 64, 6, 4, 3, False),    # likewise, 16 lanes per descent
    ({"kind": "mnk", "n": 8, "k": 4}, 8, 6, 1, 6, False),     # A = 64, one descent: the register ply at its limit
    ({"kind": "mnk", "n": 9, "k": 5}, 8, 6, 1, 6, False),     # A = 81, one descent: the one-wavefront block ply
    ({"kind": "mnk", "n": 15, "k": 5}, 4, 4, 8, 6, True),     # eight wavefronts per game: k_tree_mw, k_tree_stag_mw
]


@pytest.mark.parametrize("d,G,S,B,sbt0,evict", FORMS, ids=["c4", "mnk-3-3", "mnk-8-4", "mnk-9-5", "mnk-15-5"])
def test_all_launch_forms_agree(d, G, S, B, sbt0, evict):
    """test 3: the step-wise kernels, the fused lock-step search, the one-call move and the staggered stream play the same
    games with the same pruned tuples and the same tallies"""
    ref, st0, c0 = _run(d, G, S, B, sbt0, 11, "stepwise", k=2.0, evict=evict)
    assert st0["forced_descents"] > 0 and st0["pruned_plies"] > 0 and st0["visits_removed"] > 0
    off, _, _ = _run(d, G, S, B, sbt0, 11, "fused", evict=evict)
    assert any(not np.array_equal(ref[u]["states"], off[u]["states"]) for u in ref), "the feature changed no game"
    for form in ("fused", "move", "stag"):
        got, st, c = _run(d, G, S, B, sbt0, 11, form, k=2.0, evict=evict)
        _same(ref, got, form)
        assert st == st0, (form, st, st0)
        assert c["sims"] == c0["sims"] and c["plies"] == c0["plies"]


@pytest.mark.parametrize("d,G,S,B,sbt0,evict", [FORMS[0], FORMS[4]], ids=["c4", "mnk-15-5"])
def test_early_stop_and_resignation_compose(d, G, S, B, sbt0, evict):
    """test 4, whole games: with early stop and resignation on the lock-step and the staggered forms still agree -- moves,
    minibatch counts, root Q --, plies are cut, games are resigned, and tau = 0 tuples stay one-hot"""
    kw = dict(k=2.0, evict=evict, early=1, resign=(-0.3, 0.25))
    a, sa, _ = _run(d, G, S, B, sbt0, 12, "move", **kw)
    b, sb, _ = _run(d, G, S, B, sbt0, 12, "stag", **kw)
    _same(a, b, "staggered")
    assert sa == sb and sa["pruned_plies"] > 0
    if d is C4:  # (64 games: some plies are cut, some games resigned; four 15 x 15 games promise neither)
        assert any((g["mb"] < S).any() for g in a.values()) and any(g["resigned"] for g in a.values())
    for g in a.values():
        for i in range(sbt0, len(g["pi"])):
            assert sorted(g["pi"][i].tolist())[-2:] == [0.0, 1.0]


def test_games_start_from_their_openings():
    """test 4, openings: every game's first tuple is the opened root"""
    game = _game_of(C4)
    games, st, _ = _run(C4, 32, 5, 8, 6, 13, "stag", k=2.0, openings=4)
    assert st["forced_descents"] > 0 and st["pruned_plies"] > 0
    made = 0
    for uid, g in games.items():
        state, player, n = host_opening(game, 13, uid, uid & 1, 4)
        assert game.from_keys(np.ascontiguousarray(g["states"][:1]).view(np.uint64))[0] == state
        assert int(g["players"][0]) == player and int(g["open"][0]) == n
        made += n > 0
    assert made >= 16


@pytest.mark.parametrize("form", ["stag", "move"])
def test_restart_keeps_k_and_zero_after_two_is_off(form):
    """test 4: caro_engine_restart keeps the setting; k = 0 after k = 2 plays the off engine's games bit for bit"""
    on, st_on, _ = _run(C4, 32, 5, 8, 6, 14, form, k=2.0)
    again, st_again, _ = _run(C4, 32, 5, 8, 6, 14, form, k=2.0, restart=True)
    _same(on, again, "restarted")
    assert st_again == st_on and st_on["forced_descents"] > 0  # (the restart cleared the tallies, the run refilled them)
    off, st_off, c_off = _run(C4, 32, 5, 8, 6, 14, form)
    zero, st_zero, c_zero = _run(C4, 32, 5, 8, 6, 14, form, k=[2.0, 0.0])
    _same(off, zero, "k = 0 after k = 2")
    assert c_off == c_zero and st_off == st_zero and st_zero["root_descents"] == 0


def test_off_is_off():
    """test 5: an engine that never heard of the feature and one set to 0: 256 staggered Connect4 slots, every drain and
    the counters identical"""
    def run(k):
        eng = _engine(_game_of(C4), 256, 5, 8, 6, 15, stagger=True, n_games=256)
        if k is not None:
            eng.set_forced_playouts(k)
            assert eng.forced_playouts is None
        drains = []
        for _ in range(30):
            eng.search(5, 8)
            drains.append({kk: v.cpu().numpy().copy() for kk, v in eng.drain(recycle=False).items()})
        c, st = eng.counters(), fp.stats(eng)
        eng.close()
        return drains, c, st
    a, ca, sa = run(None)
    b, cb, sb = run(0.0)
    assert ca == cb and sa == sb and sa["root_descents"] == 0 and ca["finished"] > 0
    for x, y in zip(a, b):
        assert sorted(x) == sorted(y)
        for key in x:
            np.testing.assert_array_equal(x[key], y[key], err_msg=key)


def test_set_call_errors():
    from caro_ai_amd import _lib
    eng = _engine(_game_of(C4), 8, 4, 8, 4, 1)
    L = eng.L
    for bad in (-1.0, 64.5, float("nan")):
        assert L.caro_engine_set_forced_playouts(eng.h, bad) == -22
        with pytest.raises(ValueError):
            eng.set_forced_playouts(bad)
    sw = _Stepwise(eng, 8)
    sw.select(0, np.full((8, 8, 7), 1.0 / 7))
    assert L.caro_engine_set_forced_playouts(eng.h, 2.0) == -71  # a pending caro_select
    sw.cancel()
    eng.set_forced_playouts(2.0)
    assert eng.forced_playouts == 2.0
    eng.close()
    arena = _engine(_game_of(C4), 4, 4, 8, 0, 1, n_stores=2)  # accepted, as the playout cap is
    arena.set_forced_playouts(2.0)
    arena.search(4, 8)
    arena.step()
    assert fp.stats(arena)["root_descents"] > 0 and arena.counters()["overflows"] == 0
    arena.close()
    with pytest.raises(ValueError):
        from caro_ai_amd.lib import utils
        utils.play_games(_game_of(C4), 4, None, torch.nn.Identity(), net2=torch.nn.Identity(), forced_playouts=2,
                         device=DEV)  # an arena never uses it


# ------------------------------------------------------------------ the training path
def _shipped_net(game):
    import os
    from caro_ai_amd.lib.model import Net
    net = Net(game.obs_shape, game.action_space)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    net.load_state_dict(torch.load(os.path.join(root, "caro_ai_amd", "data", "weights", "best_026_12000.dat"),
                                   map_location="cpu"))
    return net.to(DEV).eval()


def test_self_play_reports_the_shares():
    import collections
    from caro_ai_amd import train
    from caro_ai_amd.lib import utils
    game = _game_of(C4)
    net = _shipped_net(game)

    def check(out):
        assert 0.0 < out["forced_share"] < 1.0 and 0.0 < out["pruned_visits_share"] < 1.0

    buf = train.DeviceReplayBuffer(game, 1 << 14, DEV)
    out = train.self_play(game, buf, net, 32, device=DEV, seed=3, stagger=True, forced_playouts=2)
    check(out)
    assert len(buf) > 0
    out = train.self_play_stream(game, buf, net, 32, device=DEV, seed=3, forced_playouts=2)
    check(out)
    train.release_engines()
    dq = collections.deque(maxlen=1 << 14)
    _, stats = utils.play_games(game, 16, dq, net, seed=3, device=DEV, return_stats=True, forced_playouts=2)
    check(stats)
    assert len(dq) > 0


def test_cli_forced_playouts_option_runs_and_is_logged(tmp_path, monkeypatch):
    """test 6: python -m caro_ai_amd.train --forced-playouts 2 --iterations 1 fills the replay buffer and reports"""
    from caro_ai_amd import train
    rows, lines, sizes = [], [], []

    class Writer:
        def add_scalar(self, name, value, step):
            rows.append((name, float(value), step))

        def close(self):
            pass

    deliver = train._Drains.deliver

    def spy(self, replay_buffer):
        deliver(self, replay_buffer)
        sizes.append(len(replay_buffer))

    monkeypatch.setattr(train, "_writer", lambda name: Writer())
    monkeypatch.setattr(train._Drains, "deliver", spy)
    monkeypatch.setattr("builtins.print", lambda *a, **k: lines.append(" ".join(str(x) for x in a)))
    train.main(["-n", "r", "-g", "0", "--cuda", "--games", "64", "--iterations", "1", "--saves", str(tmp_path),
                "--forced-playouts", "2"])
    got = {r[0]: r[1] for r in rows}
    assert 0.0 < got["forced_share"] < 1.0 and 0.0 < got["pruned_visits_share"] < 1.0
    assert sizes and sizes[-1] > 64
    assert any(line.startswith("Forced playouts: k 2") for line in lines)
