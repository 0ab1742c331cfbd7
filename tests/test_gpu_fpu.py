"""First-play urgency reduction on the GPU (include/caro_hip.h, "first-play urgency"; SelfPlayEngine.set_fpu): every
level of every descent of step-wise games against the numpy rule (caro_ai_amd/fpu.py) on the rows the engine holds; the
launch forms against each other; the other extensions on top of it; off is off; the set call's errors; the train path.

Every engine here evaluates with the table net (HashNet).  The boards and shapes are those of
tests/test_gpu_forced_playouts.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from caro_ai_amd import forced_playouts as fp
from caro_ai_amd import fpu
from tests.test_gpu_engine import DEV, _game_of
from tests.test_gpu_forced_playouts import (BOARDS, C4, C_PUCT, EXPLORE, FORMS, _Stepwise, _engine, _legal, _ptr, _same,
                                            _shipped_net)

pytestmark = pytest.mark.gpu

R, RR = 0.5, 0.25


class _Paths(_Stepwise):
    """_Stepwise plus the whole path (keys and actions) of every descent of the pending select"""

    def __init__(self, eng, B):
        super().__init__(eng, B)
        self.pk = torch.zeros((eng.G * B, eng.HW, eng.KW), dtype=torch.int64, device=eng.device)

    def paths(self, games):
        """{(g, b): (keys uint64[len, KW], actions int[len])}"""
        from caro_ai_amd import _lib
        eng, B = self.eng, self.B
        for g in games:
            for b in range(B):
                i = g * B + b
                _lib.check(self.L.caro_get_descent(eng.h, g, b, _ptr(self.info[i]), _ptr(self.value[i:i + 1]),
                                                   _ptr(self.leaf[i]), _ptr(self.pk[i]), _ptr(self.pact[i]),
                                                   eng._stream()))
        info = self.info.cpu().numpy()
        pk = self.pk.cpu().numpy().view(np.uint64)
        pact = self.pact.cpu().numpy()
        out = {}
        for g in games:
            for b in range(B):
                i = g * B + b
                n = int(info[i, 1])
                out[(g, b)] = (pk[i, :n].copy(), pact[i, :n].copy())
        return out


def _lookup_keys(eng, games, stores, keys):
    """caro_lookup_nodes on raw keys -> dict of numpy arrays"""
    from caro_ai_amd import _lib
    M, dev = len(games), eng.device
    g = torch.as_tensor(games, dtype=torch.int32).to(dev)
    s = torch.as_tensor(stores, dtype=torch.int32).to(dev)
    k = torch.from_numpy(np.ascontiguousarray(keys).view(np.int64)).to(dev)
    found = torch.zeros(M, dtype=torch.int32, device=dev)
    N = torch.zeros((M, eng.A), dtype=torch.int32, device=dev)
    strong = torch.zeros((M, eng.A), dtype=torch.int32, device=dev)
    W = torch.zeros((M, eng.A), dtype=torch.float32, device=dev)
    Q, P = torch.zeros_like(W), torch.zeros_like(W)
    _lib.check(eng.L.caro_lookup_nodes(eng.h, M, _ptr(g), _ptr(s), _ptr(k), _ptr(found), _ptr(N), _ptr(W), _ptr(Q), _ptr(P),
                                       _ptr(strong), eng._stream()))
    return {"found": found.cpu().numpy(), "N": N.cpu().numpy(), "W": W.cpu().numpy(), "Q": Q.cpu().numpy(),
            "P": P.cpu().numpy(), "strong": strong.cpu().numpy()}


def _check_paths(eng, game, paths, players, nz, r, rr, legal_cache, fk=0.0, tally=None, two_stores=False):
    """every action on every path is the rule's choice on the frozen tree's row, q_up chained level by level.  With
    `tally`, also counts the levels (root / below) where the rule with reduction 0 would have chosen otherwise."""
    items = [(g, b, i) for (g, b), (keys, acts) in sorted(paths.items()) for i in range(len(acts))]
    if not items:
        return
    keys = np.stack([paths[(g, b)][0][i] for g, b, i in items])
    rows = _lookup_keys(eng, [g for g, _, _ in items], [int(players[g]) if two_stores else 0 for g, _, _ in items], keys)
    assert rows["found"].all()
    at = {it: j for j, it in enumerate(items)}
    for (g, b), (pkeys, acts) in sorted(paths.items()):
        q_up = np.float32(0.0)
        for i, a in enumerate(acts):
            j = at[(g, b, i)]
            kb = pkeys[i].tobytes()
            if kb not in legal_cache:
                legal_cache[kb] = _legal(game, pkeys[i])
            legal = legal_cache[kb]
            root = i == 0
            N, W, Q, P, strong = (rows[x][j] for x in ("N", "W", "Q", "P", "strong"))
            args = (root, N, W, Q, P, strong, legal, nz[g, b] if root else None, C_PUCT, EXPLORE, q_up)
            want = fpu.level_choice(*args, rr if root else r)
            forced = False
            if root and fk > 0.0:
                f = fp.forced_root(N, P, nz[g, b], legal, EXPLORE, fk)
                if f.any():
                    want, forced = int(np.argmax(f)), True
            assert int(a) == want, (g, b, i, int(a), want, forced)
            if tally is not None:
                tally["levels"] += 1
                if not forced and fpu.level_choice(*args, 0.0) != want:
                    tally["root" if root else "below"] += 1
            q_up = fpu.raw_q_up(root, int(a), N, W, Q, strong)


def _stepwise_levels(d, G, S, B, plies, sbt0, seed, evict=False, fk=0.0, two_stores=False):
    """`plies` plies of G step-wise games; every minibatch selected twice from the same noise rows (0 / 0, cancelled; then
    R / RR) and every level of every descent of both selects checked against the numpy rule"""
    game = _game_of(d)
    kw = {"n_stores": 2} if two_stores else {}
    eng = _engine(game, G, S, B, sbt0, seed, evict=evict, **kw)
    if fk > 0.0:
        eng.set_forced_playouts(fk)
    sw = _Paths(eng, B)
    seen = dict(levels=0, root=0, below=0, stores=set())
    alive = np.ones(G, bool)
    legal_cache = {}
    for _ in range(plies):
        _, players, ply, uid = eng.roots()
        games = np.flatnonzero(alive).tolist()
        if not games:
            break
        seen["stores"].update(int(players[g]) for g in games)
        for mb in range(S):
            nz = sw.noise(uid, ply, mb)
            eng.set_fpu(0.0, 0.0)
            assert eng.kernel_form() == (1 if fk > 0.0 or two_stores else 0)
            sw.select(mb, nz)
            _check_paths(eng, game, sw.paths(games), players, nz, 0.0, 0.0, legal_cache, fk=fk, two_stores=two_stores)
            sw.cancel()
            eng.set_fpu(R, RR)
            sw.select(mb, nz)
            _check_paths(eng, game, sw.paths(games), players, nz, R, RR, legal_cache, fk=fk, tally=seen,
                         two_stores=two_stores)
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
    print("fpu, step-wise:", d, {x: seen[x] for x in ("levels", "root", "below")})
    assert seen["root"] + seen["below"] > 0, "the rule changed no choice"
    assert seen["below"] > 0, "the rule changed no choice below the root"


def test_levels_with_forced_playouts_on_top():
    """test 3, the per-level half: a forced action wins the root level, every other choice follows the rule"""
    seen = _stepwise_levels(C4, 8, 6, 4, 6, 4, 4, fk=2.0)
    print("fpu with forced playouts, step-wise:", {x: seen[x] for x in ("levels", "root", "below")})
    assert seen["root"] + seen["below"] > 0 and seen["below"] > 0


# ------------------------------------------------------------------ whole games through every launch form
def _run(d, G, S, B, sbt0, seed, form, fpu_calls=(), evict=False, forced=None, early=None, resign=None, cap=None,
         openings=None, restart=False, forms_seen=None):
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
    if forms_seen is not None:
        forms_seen.append(eng.kernel_form())
    for pair in fpu_calls:
        eng.set_fpu(*pair)
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
    """test 2: the step-wise kernels, the fused lock-step search, the one-call move and the staggered stream play the same
    games with the same tuples and the same counters"""
    ref, c0 = _run(d, G, S, B, sbt0, 21, "stepwise", [(R, RR)], evict=evict)
    off, _ = _run(d, G, S, B, sbt0, 21, "fused", evict=evict)
    assert any(not np.array_equal(ref[u]["states"], off[u]["states"]) for u in ref), "the feature changed no game"
    for form in ("fused", "move", "stag"):
        got, c = _run(d, G, S, B, sbt0, 21, form, [(R, RR)], evict=evict)
        _same(ref, got, form)
        assert c["sims"] == c0["sims"] and c["plies"] == c0["plies"]


@pytest.mark.parametrize("d,G,S,B,sbt0,evict", [FORMS[0], FORMS[4]], ids=["c4", "mnk-15-5"])
def test_the_other_options_compose(d, G, S, B, sbt0, evict):
    """test 3, whole games: forced playouts, resignation, early stop, the playout cap and openings on top.  The forms that
    know a ply's budget -- the fused search, the one-call move, the staggered stream -- agree with all five on.  A
    step-wise host loop knows no budget: early stop never cuts there (include/caro_hip.h, "early stop"), and with the
    playout cap it does not play the fused search's games with the feature off either, so the step-wise kernels are
    compared with the other three on."""
    kw = dict(evict=evict, forced=2.0, resign=(-0.2, 0.25), early=1, cap=(0.5, 2), openings=3)
    ref, c0 = _run(d, G, S, B, sbt0, 22, "fused", [(R, RR)], **kw)
    off, _ = _run(d, G, S, B, sbt0, 22, "fused", **kw)
    assert any(not np.array_equal(ref[u]["states"], off[u]["states"]) for u in ref), "the feature changed no game"
    for form in ("move", "stag"):
        got, c = _run(d, G, S, B, sbt0, 22, form, [(R, RR)], **kw)
        _same(ref, got, form)
        assert c["sims"] == c0["sims"] and c["plies"] == c0["plies"]
    kw["early"] = kw["cap"] = None
    ref, c0 = _run(d, G, S, B, sbt0, 22, "stepwise", [(R, RR)], **kw)
    got, c = _run(d, G, S, B, sbt0, 22, "fused", [(R, RR)], **kw)
    _same(ref, got, "fused, without early stop and the cap")
    assert c["sims"] == c0["sims"] and c["plies"] == c0["plies"]


@pytest.mark.parametrize("form", ["stag", "fused"])
def test_off_is_off_and_restart_keeps_the_setting(form):
    """test 4"""
    never, c_never = _run(C4, 32, 5, 8, 6, 23, form)
    forms = []
    back, c_back = _run(C4, 32, 5, 8, 6, 23, form, [(R, RR), (0.0, 0.0)], forms_seen=forms)
    assert forms == [0, 1, 0]
    _same(never, back, "0 / 0 after 0.5 / 0.25")
    assert c_never == c_back
    on, c_on = _run(C4, 32, 5, 8, 6, 23, form, [(R, RR)])
    forms = []
    again, c_again = _run(C4, 32, 5, 8, 6, 23, form, [(R, RR)], restart=True, forms_seen=forms)
    assert forms == [0, 1, 1]
    _same(on, again, "restarted")
    assert c_on == c_again
    assert any(not np.array_equal(on[u]["states"], never[u]["states"]) for u in on)


def test_set_call_errors_and_two_stores():
    """test 5"""
    eng = _engine(_game_of(C4), 8, 4, 8, 4, 1)
    L = eng.L
    for bad in ((-0.1, 0.0), (0.0, -0.1), (2.5, 0.0), (0.0, 2.5), (float("nan"), 0.0), (0.0, float("nan"))):
        assert L.caro_engine_set_fpu(eng.h, *bad) == -22
        with pytest.raises(ValueError):
            eng.set_fpu(*bad)
    assert eng.fpu is None and eng.kernel_form() == 0
    sw = _Stepwise(eng, 8)
    sw.select(0, np.full((8, 8, 7), 1.0 / 7))
    assert L.caro_engine_set_fpu(eng.h, R, RR) == -71  # a pending caro_select
    sw.cancel()
    eng.search(4, 8)
    eng.step()
    eng.drain_begin(False)
    assert L.caro_engine_set_fpu(eng.h, R, RR) == -71  # a drain pending
    eng.drain_end()
    eng.set_fpu(R)
    assert eng.fpu == (R, R)
    eng.set_fpu(R, RR)
    assert eng.fpu == (R, RR) and eng.kernel_form() == 1
    eng.close()
    seen = _stepwise_levels(C4, 4, 4, 8, 4, 0, 2, two_stores=True)  # accepted on an arena-form engine: both stores
    print("fpu, two stores:", {x: seen[x] for x in ("levels", "root", "below")})
    assert seen["stores"] == {0, 1} and seen["levels"] > 0 and seen["root"] + seen["below"] > 0


# ------------------------------------------------------------------ the training path
def test_self_play_with_fpu():
    """test 6: tuples, zero overflows (self_play raises on one)"""
    from caro_ai_amd import train
    game = _game_of(C4)
    net = _shipped_net(game)
    buf = train.DeviceReplayBuffer(game, 1 << 14, DEV)
    out = train.self_play(game, buf, net, 32, device=DEV, seed=3, stagger=True, fpu=(R, RR))
    assert len(buf) > 32 and out["steps"] > 0
    n = len(buf)
    out = train.self_play_stream(game, buf, net, 32, device=DEV, seed=3, fpu=(R, RR))
    assert len(buf) > n and out["steps"] > 0
    train.release_engines()


def test_cli_fpu_option_runs_and_is_logged(tmp_path, monkeypatch):
    """test 6: python -m caro_ai_amd.train --fpu-reduction 0.5 --fpu-root-reduction 0.25 --iterations 1"""
    from caro_ai_amd import train
    lines, sizes = [], []

    class Writer:
        def add_scalar(self, name, value, step):
            pass

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
                "--fpu-reduction", "0.5", "--fpu-root-reduction", "0.25"])
    assert sizes and sizes[-1] > 64
    assert sum(line == "First-play urgency: reduction 0.5, root reduction 0.25" for line in lines) == 1
