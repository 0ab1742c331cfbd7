"""Move temperature and visit-count policy targets on the GPU (include/caro_hip.h, "temperature";
SelfPlayEngine.set_temperature): every ply of lock-step games against the numpy rule (caro_ai_amd/temperature.py) on the
counts the engine holds; visit targets against an untouched engine; the launch forms against each other; forced
playouts and early stop on top; off is off; the training path.

Every engine here but the training path's evaluates with the table net (HashNet).  Comparisons are bit for bit.  The
lock-step games are those of uids 0 .. G-1; once the plies under test are made every mover resigns (threshold 1), so a
drain hands out the tuples without the boards being played to the end."""
import functools

import numpy as np
import pytest

from caro_ai_amd import forced_playouts as fp
from caro_ai_amd import temperature as tp
from oracle.oracle import sample_index
from tests.test_gpu_engine import DEV, _game_of
from tests.test_gpu_forced_playouts import C4, C_PUCT, FORMS, _Stepwise, _engine, _same

pytestmark = pytest.mark.gpu

IDS = ["c4", "mnk-3-3", "mnk-8-4", "mnk-9-5", "mnk-15-5"]
TRIPLES = [(1.0, 0.0, True), (0.5, 0.25, False), (2.0, 0.5, True)]


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _lockstep(i, triple, plies, seed=31, forced=None, cap=None, rows=False):
    """`plies` plies of the games of FORMS[i] through the lock-step loop (fused search, caro_policy, caro_step), then a
    ply at which every mover resigns, then the drain.  triple: None = an engine never told of the feature.  Returns, per
    uid, the per-ply records (step, N, caro_policy's pi, action[, root row]) and the drained game (resign.split_games).
    Cached: the tests share the runs and do not change them."""
    from caro_ai_amd.resign import split_games
    d, G, S, B, sbt0, evict = FORMS[i]
    game = _game_of(d)
    eng = _engine(game, G, S, B, sbt0, seed, evict=evict)
    eng.set_resign(-1.0, 0.0)  # (recording alone: Q >= -1 never resigns)
    if forced is not None:
        eng.set_forced_playouts(forced)
    if cap is not None:
        eng.set_playout_cap(*cap)
    if triple is not None:
        eng.set_temperature(*triple)
        assert eng.temperature == triple and eng.kernel_form() == 1
    seen = {g: [] for g in range(G)}
    alive = np.ones(G, bool)
    for ply_no in range(plies + 1):
        if ply_no == plies:
            eng.set_resign(1.0, 0.0)  # the closing ply: q < 1 resigns (a q of exactly 1 plays its winning move)
        keys, players, ply, uid = eng.roots()
        eng.search(S, B)
        pi, counts = eng.policy()
        pi, counts = pi.cpu().numpy(), counts.cpu().numpy()
        row = eng.lookup(list(range(G)), [0] * G, game.from_keys(keys)) if rows else None
        actions, done, _ = eng.step()
        actions, done = actions.cpu().numpy(), done.cpu().numpy()
        for g in np.flatnonzero(alive):
            assert int(uid[g]) == g
            rec = dict(step=int(ply[g]), N=counts[g].astype(np.int64), pi=pi[g].copy(), action=int(actions[g]),
                       closing=ply_no == plies)
            if rows:
                rec["row"] = {k: row[k][g].copy() for k in ("N", "W", "Q", "P", "strong")}
            seen[g].append(rec)
        alive &= done == 0
    out = eng.drain(recycle=False)
    c = eng.counters()
    eng.close()
    assert c["overflows"] == 0 and not alive.any()
    games = {g["uid"]: g for g in split_games({k: v.cpu().numpy() for k, v in out.items()})}
    assert sorted(games) == list(range(G))
    return seen, games, seed


# ------------------------------------------------------------------ 1: every ply follows the rule
@pytest.mark.parametrize("triple", TRIPLES, ids=["1-0-vt", "0.5-0.25", "2-0.5-vt"])
@pytest.mark.parametrize("i", range(5), ids=IDS)
def test_every_ply_follows_the_rule(i, triple):
    """the action is sample_index(T(N, tau_m), the move uniform), caro_policy's pi is T(N, tau_m), the drained tuple's pi
    is T(N, tau_t)"""
    from caro_ai_amd import _lib
    L = _lib.load()
    sbt0 = FORMS[i][4]
    seen, games, seed = _lockstep(i, triple, sbt0 + 3)
    early = late = differ = 0
    for uid, recs in seen.items():
        gm = games[uid]
        assert len(gm["pi"]) == len(recs)
        for k, r in enumerate(recs):
            assert r["step"] == k and r["N"].sum() > 0
            tau_m, tau_t = tp.ply_temperatures(k, sbt0, *triple)
            pm, pt = tp.policy(r["N"], tau_m), tp.policy(r["N"], tau_t)
            assert np.array_equal(_bits(r["pi"]), _bits(pm)), (uid, k, "caro_policy")
            assert np.array_equal(_bits(gm["pi"][k]), _bits(pt)), (uid, k, "the tuple")
            a = sample_index(pm, L.caro_host_move_uniform(seed, uid, k))
            assert r["action"] == a or (r["closing"] and r["action"] == _lib.RESIGNED), (uid, k)
            early += k < sbt0
            late += k >= sbt0
            differ += not np.array_equal(pm, pt)
    print("temperature, lock-step:", FORMS[i][0], triple, dict(early=early, late=late, differ=differ))
    assert early > 0 and late > 0 and (differ > 0 or not triple[2])


# ------------------------------------------------------------------ 2: visit targets do not move the games
@pytest.mark.parametrize("i", range(5), ids=IDS)
def test_visit_targets_do_not_move_the_games(i):
    sbt0 = FORMS[i][4]
    on_seen, on, _ = _lockstep(i, (1.0, 0.0, True), sbt0 + 3)
    off_seen, off, _ = _lockstep(i, None, sbt0 + 3)
    late = soft = 0
    for uid in off:
        a, b = off[uid], on[uid]
        assert [r["action"] for r in off_seen[uid]] == [r["action"] for r in on_seen[uid]]
        for key in ("states", "players", "z", "q"):
            np.testing.assert_array_equal(a[key], b[key], err_msg="%s of uid %d" % (key, uid))
        assert [a[x] for x in ("first", "result", "steps")] == [b[x] for x in ("first", "result", "steps")]
        for k, r in enumerate(on_seen[uid]):
            np.testing.assert_array_equal(r["N"], off_seen[uid][k]["N"])
            if k < sbt0:
                assert np.array_equal(_bits(a["pi"][k]), _bits(b["pi"][k]))
                continue
            late += 1
            N = r["N"]
            assert np.array_equal(_bits(b["pi"][k]), _bits(N.astype(np.float64) / np.float64(int(N.sum()))))
            assert sorted(a["pi"][k].tolist())[-2:] == [0.0, 1.0]  # the untouched engine's late tuple is one-hot
            if not r["closing"] or r["action"] >= 0:
                assert int(np.argmax(b["pi"][k])) == r["action"] == int(np.argmax(a["pi"][k]))
            soft += int((b["pi"][k] != 0).sum() > 1)
    assert late > 0 and soft > 0, "no late tuple carries a visit distribution"


# ------------------------------------------------------------------ 3: all launch forms agree
def _run(d, G, S, B, sbt0, seed, form, calls=(), evict=False, forced=None, early=None, resign=None, cap=None,
         openings=None, fpu=None, vl=None, restart=False, forms_seen=None):
    """the games of uids 0 .. G-1 played to the end through one launch form -> ({uid: game}, counters); `calls`: the
    set_temperature calls, in order"""
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
    if fpu is not None:
        eng.set_fpu(*fpu)
    if vl is not None:
        eng.set_virtual_loss(vl)
    if forms_seen is not None:
        forms_seen.append(eng.kernel_form())
    for triple in calls:
        eng.set_temperature(*triple)
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


ON = (0.5, 0.25, True)


@pytest.mark.parametrize("d,G,S,B,sbt0,evict", FORMS, ids=IDS)
def test_all_launch_forms_agree(d, G, S, B, sbt0, evict):
    """the step-wise kernels, the fused lock-step search, the one-call move and the staggered stream play the same games
    with the same tuples.  The forms that know a ply's budget agree with every other option on; a step-wise host loop
    knows no budget -- early stop never cuts there, and under the playout cap it does not play the fused search's games
    with this feature off either (tests/test_gpu_fpu.py) --, so it is compared with the other options but those two."""
    kw = dict(evict=evict, forced=2.0, resign=(-0.2, 0.25), early=1, cap=(0.5, 2), openings=3, fpu=(0.5, 0.25), vl=2)
    ref, c0 = _run(d, G, S, B, sbt0, 32, "fused", [ON], **kw)
    off, _ = _run(d, G, S, B, sbt0, 32, "fused", **kw)
    assert any(not np.array_equal(ref[u]["states"], off[u]["states"]) for u in ref), "the feature changed no game"
    for form in ("move", "stag"):
        got, c = _run(d, G, S, B, sbt0, 32, form, [ON], **kw)
        _same(ref, got, form)
        assert c["sims"] == c0["sims"] and c["plies"] == c0["plies"]
    kw["early"] = kw["cap"] = None
    ref, c0 = _run(d, G, S, B, sbt0, 32, "stepwise", [ON], **kw)
    got, c = _run(d, G, S, B, sbt0, 32, "fused", [ON], **kw)
    _same(ref, got, "fused, without early stop and the cap")
    assert c["sims"] == c0["sims"] and c["plies"] == c0["plies"]
    soft = sum(int(((g["pi"][sbt0:] != 0).sum(axis=1) > 1).sum()) for g in ref.values())
    assert soft > 0, "no late tuple carries a visit distribution"


# ------------------------------------------------------------------ 4: composition
def test_forced_playouts_prune_the_late_full_plies_too():
    """forced playouts on, playout cap (0.5, 2), visit targets: the pi of a full ply, early or late, is T(N', 1) with N'
    from forced_playouts.py; a fast ply is unpruned; the move comes from the unpruned counts"""
    from caro_ai_amd import _lib
    L = _lib.load()
    sbt0, cap, k = FORMS[0][4], (0.5, 2), 2.0
    seen, games, seed = _lockstep(0, (1.0, 0.0, True), sbt0 + 4, seed=33, forced=k, cap=cap, rows=True)
    tally = dict(late_full=0, late_pruned=0, late_fast=0, early_pruned=0)
    for uid, recs in seen.items():
        gm = games[uid]
        for i, r in enumerate(recs):
            N, row = r["N"], r["row"]
            np.testing.assert_array_equal(N, row["N"].astype(np.int64))
            fast = not L.caro_host_cap_uniform(seed, uid, i) < cap[0]
            assert bool(gm["full"][i]) == (not fast)
            tau_m, tau_t = tp.ply_temperatures(i, sbt0, 1.0, 0.0, True)
            assert tau_t == 1.0
            n2 = N
            if not fast:
                q = fp.edge_q(row["N"], row["W"], row["Q"], row["strong"])
                n2, _ = fp.prune(N, q, row["P"], C_PUCT, k)
                n2 = np.asarray(n2, np.int64)
            assert np.array_equal(_bits(gm["pi"][i]), _bits(tp.policy(n2, 1.0))), (uid, i, fast)
            pm = tp.policy(N, tau_m)
            a = sample_index(pm, L.caro_host_move_uniform(seed, uid, i))
            assert r["action"] == a or (r["closing"] and r["action"] == _lib.RESIGNED)
            pruned = int(n2.sum()) < int(N.sum())
            if i >= sbt0:
                tally["late_full"] += not fast
                tally["late_fast"] += fast
                tally["late_pruned"] += pruned
            else:
                tally["early_pruned"] += pruned
    print("temperature with forced playouts and the cap:", tally)
    assert tally["late_full"] > 0 and tally["late_fast"] > 0 and tally["late_pruned"] > 0 and tally["early_pruned"] > 0


def test_early_stop_never_cuts_under_visit_targets_and_cuts_as_ever_when_off():
    d, G, S, B, sbt0, evict = FORMS[0]
    never, c_never = _run(d, G, S, B, sbt0, 34, "move", early=1)
    assert any((g["mb"] < S).any() for g in never.values()), "the untouched engine cut no ply"
    back, c_back = _run(d, G, S, B, sbt0, 34, "move", [(1.0, 0.0, True), (1.0, 0.0, False)], early=1)
    _same(never, back, "(1, 0, False): early stop as on an untouched engine")
    assert c_never == c_back
    for form in ("move", "stag"):
        on, _ = _run(d, G, S, B, sbt0, 34, form, [(1.0, 0.0, True)], early=1)
        for g in on.values():
            assert (g["mb"] == S).all(), "a ply was cut under visit targets"
    soft, _ = _run(d, G, S, B, sbt0, 34, "move", [(1.0, 0.25, False)], early=1)  # a positive late temperature
    for g in soft.values():
        assert (g["mb"] == S).all(), "a ply at a positive temperature was cut"


# ------------------------------------------------------------------ 5: off is off
@pytest.mark.parametrize("form", ["stag", "fused"])
def test_off_is_off_and_restart_keeps_the_setting(form):
    d, G, S, B, sbt0, evict = FORMS[0]
    never, c_never = _run(d, G, S, B, sbt0, 35, form)
    forms = []
    back, c_back = _run(d, G, S, B, sbt0, 35, form, [ON, (1.0, 0.0, False)], forms_seen=forms)
    assert forms == [0, 1, 0]
    assert sorted(never) == sorted(back) and c_never == c_back
    for uid in never:
        for key in ("states", "players", "pi", "z"):
            assert never[uid][key].tobytes() == back[uid][key].tobytes(), (key, uid)
        assert [never[uid][x] for x in ("first", "result", "steps")] == [back[uid][x] for x in ("first", "result", "steps")]
    on, c_on = _run(d, G, S, B, sbt0, 35, form, [ON])
    forms = []
    again, c_again = _run(d, G, S, B, sbt0, 35, form, [ON], restart=True, forms_seen=forms)
    assert forms == [0, 1, 1]
    _same(on, again, "restarted")
    assert c_on == c_again
    assert any(not np.array_equal(on[u]["states"], never[u]["states"]) for u in on)


def test_set_call_errors():
    eng = _engine(_game_of(C4), 8, 4, 8, 4, 1)
    L = eng.L
    nan = float("nan")
    for bad in ((-1.0, 0.0, 0), (1.0, -0.5, 0), (0.01, 0.0, 0), (1.0, 0.049, 0), (8.5, 0.0, 0), (1.0, 9.0, 0),
                (nan, 0.0, 0), (1.0, nan, 0), (1.0, 0.0, 2), (1.0, 0.0, -1)):
        assert L.caro_engine_set_temperature(eng.h, *bad) == -22, bad
        with pytest.raises(ValueError):
            eng.set_temperature(*bad)
    assert eng.temperature is None and eng.kernel_form() == 0
    sw = _Stepwise(eng, 8)
    sw.select(0, np.full((8, 8, 7), 1.0 / 7))
    assert L.caro_engine_set_temperature(eng.h, 0.5, 0.25, 1) == -71  # a pending caro_select
    sw.cancel()
    eng.search(4, 8)
    eng.step()
    eng.drain_begin(False)
    assert L.caro_engine_set_temperature(eng.h, 0.5, 0.25, 1) == -71  # a drain pending
    eng.drain_end()
    for ok in ((0.0, 0.0, False), (0.05, 8.0, True), (8.0, 0.05, False), (1.0, 0.0, True)):
        eng.set_temperature(*ok)
        assert eng.temperature == ok and eng.kernel_form() == 1
    eng.set_temperature()
    assert eng.temperature is None and eng.kernel_form() == 0
    eng.close()
    arena = _engine(_game_of(C4), 4, 4, 8, 0, 1, n_stores=2)  # accepted on an engine with two stores, as the others are
    arena.set_temperature(1.0, 0.5, True)
    arena.search(4, 8)
    arena.step()
    assert arena.counters()["overflows"] == 0
    arena.close()


# ------------------------------------------------------------------ 6: the training path
def _shipped_c4_net(game, name="best_025_10600.dat"):
    import os
    import torch
    from caro_ai_amd.lib.model import Net
    net = Net(game.obs_shape, game.action_space)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    net.load_state_dict(torch.load(os.path.join(root, "caro_ai_amd", "data", "weights", name), map_location="cpu"))
    return net.to(DEV).eval()


def test_self_play_reports_the_onehot_share():
    """64 Connect4 games at 4 x 8 simulations with a shipped net.  Off: more than 0.4 of the tuples are one-hot; with
    visit targets strictly fewer (a late ply whose search visited one child only is still one-hot: not zero).
    The off share is a property of the games an engine without the feature plays, and they are fixed by (net, seed).
    Measured on an MI355X over seeds 0 .. 5, lock-step and staggered alike: best_025_10600 0.426 .. 0.489 (0.4466 at the
    seed used here), best_026_12000 0.396 .. 0.454 -- at 32 simulations a ply its games average 16.4 plies, ten of them
    early, so the 0.4 is not guaranteed by that net (seed 3: 0.3957).  With visit targets: 0.046 .. 0.070 and
    0.019 .. 0.026.  Hence best_025_10600 and seed 0."""
    from caro_ai_amd import train
    game = _game_of(C4)
    net = _shipped_c4_net(game)
    buf = train.DeviceReplayBuffer(game, 1 << 14, DEV)
    kw = dict(device=DEV, seed=0, stagger=True, searches=4, batch=8)
    off = train.self_play(game, buf, net, 64, **kw)
    assert off["onehot_share"] > 0.4
    on = train.self_play(game, buf, net, 64, temperature=(1.0, 0.0, True), **kw)
    print("onehot_share: off %.4f, visit targets %.4f" % (off["onehot_share"], on["onehot_share"]))
    assert on["onehot_share"] < off["onehot_share"]
    assert on["games"] == 64 and on["steps"] == off["steps"]  # (visit targets do not move the games)
    n = len(buf)
    out = train.self_play_stream(game, buf, net, 64, device=DEV, seed=0, searches=4, batch=8,
                                 temperature=(1.0, 0.25, True))
    assert len(buf) > n and 0.0 <= out["onehot_share"] < off["onehot_share"]
    again = train.self_play(game, buf, net, 64, **kw)  # an engine without the feature is kept apart from one with it
    assert again["onehot_share"] == off["onehot_share"]
    train.release_engines()


def test_cli_temperature_options_run_and_are_logged(tmp_path, monkeypatch):
    """python -m caro_ai_amd.train --visit-targets --tau-late 0.25 --iterations 1"""
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
                "--visit-targets", "--tau-late", "0.25"])
    got = {r[0]: r[1] for r in rows}
    assert 0.0 <= got["onehot_share"] < 0.4
    assert sizes and sizes[-1] > 64
    assert sum(line == "Temperature: early 1, late 0.25, targets visit counts" for line in lines) == 1
