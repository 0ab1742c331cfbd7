"""The two compiled forms of the one-wave fused tree kernels (include/caro_hip.h, "form of the one-wave fused tree
kernels"; TreeOpt in caro_engine.hip): the lean form -- opt-in self-play features, second store and diagnostic stamps
compiled out -- must compute what the full form computes, bit for bit, and a launch may pick it only while the engine uses
none of what it lacks.

Every engine here evaluates with the table net (HashNet).  That the full form is still the kernel it was, and that no
engine with a feature on is handed the lean form, is what the suites of the features themselves check."""
import numpy as np
import pytest

from caro_ai_amd._lib import CaroError
from tests.test_gpu_engine import DEV, _game_of

pytestmark = pytest.mark.gpu

C4 = {"kind": "c4"}
T3 = {"kind": "mnk", "n": 3, "k": 3}


def _engine(game, G, S, B, seed, stagger, n_stores=1, grain=0):
    from caro_ai_amd.engine import SelfPlayEngine
    from caro_ai_amd.net_hip import HashNet
    evs = [HashNet(game, device=DEV, salt=0x1111 * (i + 1), grain=grain) for i in range(n_stores)]
    return SelfPlayEngine(game, G, evaluators=evs, n_stores=n_stores, max_batch=B, steps_before_tau_0=2, seed=seed,
                          device=DEV, searches_hint=S, stagger=stagger)


def _play(d, G, S, B, moves, stagger, form, grain=0):
    """`moves` moves of G games, drained (finished slots restarted) after every move: the concatenated tuples, the
    root visit counts of every slot after the last move, the counters, the uid of every slot's current game"""
    game = _game_of(d)
    eng = _engine(game, G, S, B, 21, stagger, grain=grain)
    if form:
        eng.set_kernel_form(form)
    assert eng.kernel_form() == form
    rows = {k: [] for k in ("states", "players", "pi", "z")}
    for _ in range(moves):
        eng.search(S, B)
        eng.step()
        t = eng.drain(recycle=True)
        for k in rows:
            rows[k].append(t[k].cpu().numpy().copy())
    assert eng.kernel_form() == form  # nothing on the way has changed the choice
    counts = eng.policy()[1].cpu().numpy()
    c = eng.counters()
    uid = eng.roots()[3].astype(np.int64)
    eng.close()
    return {k: np.concatenate(v) for k, v in rows.items()}, counts, c, uid


@pytest.mark.parametrize("d,G,S,B,moves,stagger,grain", [
    (C4, 16, 3, 8, 40, True, 0),    # k_tree_stag, 8 lanes per descent
    (C4, 16, 3, 8, 40, False, 0),   # k_tree
    (T3, 16, 3, 4, 30, True, 0),    # k_tree_stag, 16 lanes per descent
    (T3, 16, 3, 4, 30, False, 0),   # k_tree
    (C4, 16, 3, 8, 40, False, 1),   # k_tree with the table net's 24-bit values: float32 sums that show their order
], ids=["c4-staggered", "c4-lock-step", "ttt-staggered", "ttt-lock-step", "c4-lock-step-fine-values"])
def test_lean_form_equals_full_form_bit_for_bit(d, G, S, B, moves, stagger, grain):
    """two engines with the same seed and uids, one automatic (lean: nothing is switched on), one held in the full form:
    every tuple of every finished game, the trees' root rows and the tallies are the same bits"""
    lean = _play(d, G, S, B, moves, stagger, 0, grain)
    full = _play(d, G, S, B, moves, stagger, 1, grain)
    for side in (lean, full):
        rows, counts, c, uid = side
        # a ply, a game end, a park and a restart have all been run: games finished and their slots play the next ones
        assert c["finished"] >= 1 and rows["z"].shape[0] >= 1 and (uid >= G).any(), (c, uid)
        assert c["overflows"] == 0
    for k in ("states", "players", "pi", "z"):
        assert lean[0][k].dtype == full[0][k].dtype and lean[0][k].shape == full[0][k].shape, k
        assert np.array_equal(lean[0][k].view(np.uint8), full[0][k].view(np.uint8)), k  # bits: pi is float64
    assert np.array_equal(lean[1], full[1])
    assert lean[2] == full[2]
    assert np.array_equal(lean[3], full[3])


def test_the_choice_follows_the_engine_state():
    """no search is launched: the form is a function of the engine's state at the moment it is asked"""
    game = _game_of(C4)

    def fresh(**kw):
        return _engine(game, 4, 4, 8, 5, False, **kw)

    eng = fresh()
    assert eng.kernel_form() == 0
    eng.set_kernel_form(1)
    assert eng.kernel_form() == 1
    eng.set_kernel_form(0)
    assert eng.kernel_form() == 0
    with pytest.raises(CaroError, match="kernel form must be 0"):  # CARO_E_INVAL, the library's own error
        eng.set_kernel_form(2)
    assert eng.kernel_form() == 0
    eng.set_kernel_form(1)
    eng.restart()  # the switch is the engine's, not the run's: it survives caro_engine_restart
    assert eng.kernel_form() == 1
    eng.set_kernel_form(0)
    assert eng.kernel_form() == 0
    # diagnostic stamps: only the full form takes them
    assert eng.L.caro_debug_stamps(eng.h, 1) == 0
    assert eng.kernel_form() == 1
    assert eng.L.caro_debug_stamps(eng.h, 0) == 0
    assert eng.kernel_form() == 0
    eng.close()

    # forced playouts: the one feature a setter switches off again
    eng = fresh()
    eng.set_forced_playouts(0)  # never on: stays off
    assert eng.kernel_form() == 0
    eng.set_forced_playouts(2.0)
    assert eng.kernel_form() == 1
    eng.set_forced_playouts(0)
    assert eng.kernel_form() == 0
    eng.set_forced_playouts(1.0)
    assert eng.kernel_form() == 1
    eng.close()

    # the others stay on once set (their arrays are kept and written from then on), whatever the value
    for on in (lambda e: e.set_resign(-1.0), lambda e: e.set_playout_cap(1.0, 2), lambda e: e.set_early_stop(1),
               lambda e: e.set_openings(2)):
        eng = fresh()
        assert eng.kernel_form() == 0
        on(eng)
        assert eng.kernel_form() == 1
        eng.close()
    eng = fresh()
    eng.set_openings(0)  # never on: nothing is allocated, nothing is recorded
    assert eng.kernel_form() == 0
    eng.set_openings(2)
    eng.set_openings(0)  # the per-game opening counts are still kept for the drains: not the lean form
    assert eng.kernel_form() == 1
    eng.close()

    # an arena engine: one tree per player
    eng = fresh(n_stores=2)
    assert eng.kernel_form() == 1
    eng.close()
