"""Call-sequence refusals of the engine's C API (include/caro_hip.h): which call refuses which engine state, with which
code and which text, and which refusal comes first where two apply.  The expected strings are written out here, copied
from the library's source at the commit before the refusals were gathered behind one helper; nothing below is produced
by the code under test.  Every call is made with arguments that are valid but for the state."""
import ctypes as C

import pytest
import torch

from caro_ai_amd import _lib
from caro_ai_amd.engine import SelfPlayEngine
from caro_ai_amd.lib.game.connect_four import ConnectFour
from caro_ai_amd.net_hip import HashNet
from tests.synth_net import SynthNet

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E_INVAL, E_STATE = -22, -71
G, B, STAGGER = 2, 8, 3

SELECT = " with a pending caro_select"
DRAIN = " with a drain pending (caro_drain_tuples_end first)"
STAG = ": the engine runs in staggered mode (per-game clocks, pending minibatches, parked games); "
STAG_USE = STAG + "use caro_search_staggered / caro_drain_parked_begin"
LEVELS = ": session levels are on (caro_pool_level); the two do not combine"
NOT_STAG = "the engine was not created in staggered mode (caro_config.stagger)"

SETTERS = ("caro_engine_set_playout_cap", "caro_engine_set_early_stop", "caro_engine_set_openings",
           "caro_engine_set_forced_playouts", "caro_engine_set_fpu", "caro_engine_set_virtual_loss",
           "caro_engine_set_temperature")
LEVEL_SETTERS = ("caro_engine_set_playout_cap", "caro_engine_set_early_stop", "caro_engine_set_temperature")
POOL = ("caro_pool_open", "caro_pool_set", "caro_pool_select", "caro_pool_select_budget", "caro_pool_level",
        "caro_pool_hold")
# the calls of a lock-step engine that are no setters: what a staggered engine refuses
LOCK_STEP = ("caro_reset_games", "caro_set_roots", "caro_select", "caro_search_batch", "caro_search_move", "caro_step",
             "caro_drain_tuples_begin")


def _p(t):
    return C.c_void_p(t.data_ptr())


class Rig:
    """An engine of 2 Connect4 games, batch 8 (lock-step: a host-evaluated net, so caro_select leaves its select
    pending; staggered: the device table net), and every covered call with valid arguments."""

    def __init__(self, stagger=False):
        game = ConnectFour()
        self.net = HashNet(game, device=DEV)  # the caro_net of the caro_search_* calls
        ev = self.net if stagger else SynthNet(84, 7, DEV)
        self.eng = e = SelfPlayEngine(game, G, evaluators=[ev], max_batch=B, seed=5, device=DEV,
                                      searches_hint=STAGGER, stagger=stagger)
        self.L, self.h = e.L, e.h
        i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=DEV)
        i64 = lambda n: torch.zeros(n, dtype=torch.int64, device=DEV)
        f32 = lambda n: torch.zeros(n, dtype=torch.float32, device=DEV)
        f64 = lambda n: torch.zeros(n, dtype=torch.float64, device=DEV)
        self.keys, self.players, self.ply, self.uid = i64(G * e.KW), i32(G), i32(G), i64(G)
        assert self.L.caro_get_roots(self.h, _p(self.keys), _p(self.players), _p(self.ply), _p(self.uid), None) == 0
        self.out3 = [i32(G) for _ in range(3)]  # actions, done, result
        self.cap = cap = G * e.maxply
        self.drain_bufs = [i64(cap * e.KW), i32(cap), f64(cap * e.A), i32(cap), i64(G * 4)]
        self.extra = {"root_q": f64(cap), "full": torch.zeros(cap, dtype=torch.uint8, device=DEV),
                      "minibatches": torch.zeros(cap, dtype=torch.int16, device=DEV),
                      "open": torch.zeros(cap, dtype=torch.int16, device=DEV)}
        self.slot, self.one, self.tau = i32(1), torch.ones(1, dtype=torch.int32, device=DEV), f64(1)
        self.lines_i = [i32(1) for _ in range(7)]  # n_lines, root_visits, len, end, move, N, strong
        self.lines_f = [f32(1) for _ in range(3)]  # W, Q, P
        torch.cuda.synchronize()

    def close(self):
        torch.cuda.synchronize()
        self.eng.close()
        self.net.close()

    def search_args(self):
        e = self.eng
        return _p(e.planes), _p(e.leaf_keys), _p(e._probs), _p(e._values)

    def drain_args(self):
        return [self.h, self.cap] + [_p(t) for t in self.drain_bufs]

    def ex(self, **want):
        return C.byref(_lib.CaroDrainExtraOpen(**{k: self.extra[k].data_ptr() for k in want}))

    def call(self, name, **kw):
        """the call `name` with valid arguments; `kw` replaces one of them"""
        L, h, e = self.L, self.h, self.eng
        a = lambda key, default: kw.get(key, default)
        n_l, rv, ln, end, mv, N, strong = [_p(t) for t in self.lines_i]
        W, Q, P = [_p(t) for t in self.lines_f]
        table = {
            "caro_engine_set_resign": lambda: L.caro_engine_set_resign(h, a("threshold", -0.9), 0.1),
            "caro_engine_set_playout_cap": lambda: L.caro_engine_set_playout_cap(h, a("p_full", 0.5), a("fast", 2)),
            "caro_engine_set_early_stop": lambda: L.caro_engine_set_early_stop(h, a("min_minibatches", 2)),
            "caro_engine_set_openings": lambda: L.caro_engine_set_openings(h, a("max_plies", 2)),
            "caro_engine_set_forced_playouts": lambda: L.caro_engine_set_forced_playouts(h, a("k", 2.0)),
            "caro_engine_set_fpu": lambda: L.caro_engine_set_fpu(h, a("reduction", 0.5), 0.25),
            "caro_engine_set_virtual_loss": lambda: L.caro_engine_set_virtual_loss(h, a("n_vl", 2)),
            "caro_engine_set_temperature": lambda: L.caro_engine_set_temperature(h, a("tau_early", 0.5), 0.25, 1),
            "caro_engine_restart": lambda: L.caro_engine_restart(h, C.byref(a("cfg", e.cfg)), None),
            "caro_reset_games": lambda: L.caro_reset_games(h, None, None),
            "caro_set_roots": lambda: L.caro_set_roots(h, _p(self.keys), _p(self.players), None),
            "caro_select": lambda: L.caro_select(h, a("batch", B), 0, None, _p(e.planes), _p(e.leaf_keys), None),
            "caro_search_batch": lambda: L.caro_search_batch(h, self.net.h, None, a("searches", 2), B, None,
                                                             *self.search_args(), None),
            "caro_search_move": lambda: L.caro_search_move(h, self.net.h, None, 2, B, None, None, *self.search_args(),
                                                           *[_p(t) for t in self.out3], None),
            "caro_step": lambda: L.caro_step(h, None, *[_p(t) for t in self.out3], None),
            "caro_drain_tuples_begin": lambda: L.caro_drain_tuples_begin(*self.drain_args(), 1, None),
            "caro_drain_parked_begin": lambda: L.caro_drain_parked_begin(*self.drain_args(), None),
            "caro_principal_lines": lambda: L.caro_principal_lines(h, 1, _p(self.slot), 0, a("top", 1), 1, n_l, rv, ln,
                                                                   end, mv, N, W, Q, P, strong, None),
            "caro_pool_open": lambda: L.caro_pool_open(h, 0, _p(self.slot), _p(self.uid), _p(self.players), None),
            "caro_pool_set": lambda: L.caro_pool_set(h, 0, _p(self.slot), _p(self.keys), _p(self.players), _p(self.ply),
                                                     None),
            "caro_pool_select": lambda: L.caro_pool_select(h, 0, _p(self.slot), None),
            "caro_pool_select_budget": lambda: L.caro_pool_select_budget(h, 0, _p(self.slot), _p(self.one), None),
            "caro_pool_level": lambda: L.caro_pool_level(h, 0, _p(self.slot), _p(self.slot), _p(self.tau), None),
            "caro_pool_hold": lambda: L.caro_pool_hold(h, None),
        }
        return table[name]()

    def expect(self, name, code, text=None, **kw):
        rc = self.call(name, **kw)
        got = self.L.caro_last_error().decode()
        assert rc == code, (name, kw, rc, got)
        if code != 0:
            assert got == text, (name, kw, got)

    def select(self):
        self.expect("caro_select", 0)

    def cancel(self):
        assert self.L.caro_select_cancel(self.h) == 0

    def drain_end(self):
        n, g = C.c_int64(), C.c_int64()
        assert self.L.caro_drain_tuples_end(self.h, C.byref(n), C.byref(g)) == 0


@pytest.fixture
def rig():
    r = Rig()
    yield r
    r.close()


@pytest.fixture
def stag():
    r = Rig(stagger=True)
    yield r
    r.close()


def test_select_pending(rig):
    rig.select()
    rig.expect("caro_engine_set_resign", 0)  # (no pending check at all)
    for name in SETTERS + ("caro_engine_restart", "caro_step", "caro_principal_lines") + POOL:
        rig.expect(name, E_STATE, name + SELECT)
    rig.expect("caro_select", E_STATE, "caro_select called twice without caro_expand_backup")
    rig.expect("caro_search_batch", E_STATE, "caro_search_batch" + SELECT)
    rig.expect("caro_search_move", E_STATE, "caro_search_batch" + SELECT)  # (one body: it names caro_search_batch)
    rig.expect("caro_drain_tuples_begin", E_STATE, "caro_drain_tuples" + SELECT)
    rig.expect("caro_drain_parked_begin", E_STATE, NOT_STAG)
    rig.expect("caro_set_roots", 0)
    rig.expect("caro_reset_games", 0)  # (and the select is gone)
    rig.select()
    rig.cancel()


def test_drain_pending(rig):
    rig.expect("caro_drain_tuples_begin", 0)
    rig.expect("caro_engine_set_resign", 0)
    for name in SETTERS + ("caro_engine_restart", "caro_principal_lines") + POOL:
        rig.expect(name, E_STATE, name + DRAIN)
    rig.expect("caro_drain_tuples_begin", E_STATE, "caro_drain_tuples_begin twice without caro_drain_tuples_end")
    rig.expect("caro_drain_parked_begin", E_STATE, NOT_STAG)
    rig.select()
    rig.cancel()
    for name in ("caro_search_batch", "caro_search_move", "caro_step", "caro_set_roots", "caro_reset_games"):
        rig.expect(name, 0)
    rig.drain_end()


def test_select_and_drain_pending(rig):
    """both at once (caro_select does not look at the drain): which of the two a call names"""
    rig.expect("caro_drain_tuples_begin", 0)
    rig.select()
    for name in SETTERS + ("caro_principal_lines",) + POOL:
        rig.expect(name, E_STATE, name + SELECT)
    rig.expect("caro_engine_restart", E_STATE, "caro_engine_restart" + DRAIN)
    rig.expect("caro_drain_tuples_begin", E_STATE, "caro_drain_tuples" + SELECT)
    rig.expect("caro_engine_set_resign", 0)
    rig.cancel()
    rig.drain_end()


def test_levels_on(rig):
    rig.expect("caro_pool_select_budget", 0)  # an empty list: session levels are on, every slot held
    for name in LEVEL_SETTERS:
        rig.expect(name, E_STATE, name + LEVELS)
    rig.expect("caro_engine_set_playout_cap", E_INVAL, "playout cap p_full must be in [0, 1]", p_full=2.0)
    rig.expect("caro_drain_parked_begin", E_STATE, NOT_STAG)
    rig.select()
    rig.cancel()
    for name in ("caro_search_batch", "caro_search_move", "caro_step", "caro_principal_lines") + POOL:
        rig.expect(name, 0)
    rig.expect("caro_drain_tuples_begin", 0)
    rig.drain_end()
    for name in ("caro_engine_set_resign", "caro_engine_set_openings", "caro_engine_set_forced_playouts",
                 "caro_engine_set_fpu", "caro_engine_set_virtual_loss", "caro_set_roots", "caro_engine_restart",
                 "caro_reset_games"):
        rig.expect(name, 0)


def test_argument_or_state(rig):
    """a bad argument and a refused state at once: which one the call reports"""
    rig.select()
    for name, kw, text in (
            ("caro_engine_set_resign", {"threshold": 2.0}, "resign threshold must be in [-1, 1]"),
            ("caro_engine_set_playout_cap", {"p_full": 2.0}, "playout cap p_full must be in [0, 1]"),
            ("caro_engine_set_playout_cap", {"fast": 1},
             "playout cap fast must be >= 2 (a fast first ply must expand its root)"),
            ("caro_engine_set_early_stop", {"min_minibatches": 0}, "early stop min_minibatches must be >= 1"),
            ("caro_engine_set_openings", {"max_plies": -1}, "caro_engine_set_openings: max_plies must be in [0, 64]"),
            ("caro_engine_set_openings", {"max_plies": 42},
             "caro_engine_set_openings: max_plies must be below the board's cell count"),
            ("caro_engine_set_forced_playouts", {"k": -1.0}, "caro_engine_set_forced_playouts: k must be in [0, 64]"),
            ("caro_engine_set_fpu", {"reduction": 3.0}, "caro_engine_set_fpu: a reduction must be in [0, 2]"),
            ("caro_engine_set_virtual_loss", {"n_vl": 17}, "caro_engine_set_virtual_loss: n_vl must be in [0, 16]"),
            ("caro_engine_set_temperature", {"tau_early": 9.0},
             "caro_engine_set_temperature: a temperature must be 0 or in [0.05, 8]"),
            ("caro_select", {"batch": B + 1}, "batch exceeds max_batch of the engine"),
            ("caro_search_batch", {"searches": 0}, "searches must be >= 1")):
        rig.expect(name, E_INVAL, text, **kw)
    other = _lib.CaroConfig.from_buffer_copy(rig.eng.cfg)
    other.n_games = G + 1
    rig.expect("caro_engine_restart", E_INVAL,
               "caro_engine_restart: the configuration differs from the engine's in a field that shapes its memory "
               "(game, n_games, n_stores, n_nets, max_batch, node_cap, evict, device, staggered or not)", cfg=other)
    rig.expect("caro_principal_lines", E_STATE, "caro_principal_lines" + SELECT, top=0)  # here the state comes first
    rig.cancel()
    rig.expect("caro_principal_lines", E_INVAL, "caro_principal_lines: top must be in [1, 16]", top=0)


def test_null_engine():
    L = _lib.load()
    for name, args in (("caro_engine_set_resign", (0.0, 0.0)), ("caro_engine_set_playout_cap", (0.5, 2)),
                       ("caro_engine_set_early_stop", (2,)), ("caro_engine_set_openings", (2,)),
                       ("caro_engine_set_forced_playouts", (2.0,)), ("caro_engine_set_fpu", (0.5, 0.25)),
                       ("caro_engine_set_virtual_loss", (2,)), ("caro_engine_set_temperature", (0.5, 0.25, 1)),
                       ("caro_reset_games", (None, None)), ("caro_step", (None,) * 5), ("caro_pool_hold", (None,))):
        assert getattr(L, name)(None, *args) == E_INVAL, name
        assert L.caro_last_error() == b"null engine", name
    for name, args in (("caro_engine_restart", (None, None)), ("caro_set_roots", (None,) * 3),
                       ("caro_select", (B, 0, None, None, None, None)), ("caro_pool_select", (0, None, None))):
        assert getattr(L, name)(None, *args) == E_INVAL, name
        assert L.caro_last_error() == b"null argument", name


def test_staggered_engine(stag):
    for name in LOCK_STEP:
        who = "caro_search_batch" if name == "caro_search_move" else name
        stag.expect(name, E_STATE, who + STAG_USE)
    stag.expect("caro_principal_lines", E_STATE, "caro_principal_lines" + STAG + "the read-out is lock-step")
    for name in POOL:
        stag.expect(name, E_STATE, name + STAG + "the pool is lock-step")
    # arguments are looked at before the mode
    stag.expect("caro_select", E_INVAL, "batch exceeds max_batch of the engine", batch=B + 1)
    stag.expect("caro_search_batch", E_INVAL, "searches must be >= 1", searches=0)
    stag.expect("caro_engine_set_playout_cap", E_INVAL, "playout cap fast must be <= caro_config.stagger",
                fast=STAGGER + 1)
    stag.expect("caro_drain_parked_begin", 0)
    stag.expect("caro_drain_parked_begin", E_STATE, "caro_drain_parked_begin twice without caro_drain_tuples_end")
    for name in SETTERS:
        stag.expect(name, E_STATE, name + DRAIN)
    stag.expect("caro_engine_restart", E_STATE, "caro_engine_restart" + DRAIN)
    stag.expect("caro_engine_set_resign", 0)
    stag.drain_end()


BEFORE = (("open", ": open_dev before caro_engine_set_openings (no opening counts recorded)", "_ex"),
          ("minibatches", ": minibatches_dev before caro_engine_set_early_stop (no minibatch counts recorded)", "_ex"),
          ("root_q", " before caro_engine_set_resign (no root Q recorded)", "_q"),
          ("full", " before caro_engine_set_playout_cap (no ply classes recorded)", "_x"))


def _drains(r):
    """(name, the _ex call with a caro_drain_extra) of both drains"""
    return (("caro_drain_tuples_begin", lambda ex: r.L.caro_drain_tuples_begin_ex(*r.drain_args(), 1, ex, None)),
            ("caro_drain_parked_begin", lambda ex: r.L.caro_drain_parked_begin_ex(*r.drain_args(), ex, None)))


@pytest.mark.parametrize("which", ["rig", "stag"])
def test_drain_outputs_before_their_setters(which, request):
    """an optional output of a feature that was never set: refused by both drains, on an engine of either mode -- before
    the drain looks at the mode or at what is pending -- and in this order when several are asked for"""
    r = request.getfixturevalue(which)
    if which == "rig":
        r.select()
    for name, begin in _drains(r):
        unset = _lib.CaroDrainExtraOpen()
        unset.size = 0
        assert begin(C.byref(unset)) == E_INVAL and r.L.caro_last_error() == b"caro_drain_extra.size is not set", name
        for field, tail, suffix in BEFORE:
            assert begin(r.ex(**{field: 1})) == E_STATE, (name, field)
            assert r.L.caro_last_error().decode() == name + suffix + tail, (name, field)
        for first, (field, tail, suffix) in enumerate(BEFORE):
            assert begin(r.ex(**{f: 1 for f, _, _ in BEFORE[first:]})) == E_STATE
            assert r.L.caro_last_error().decode() == name + suffix + tail, (name, "from", field)
    # the older entry points reach the same refusals
    q, f = _p(r.extra["root_q"]), _p(r.extra["full"])
    assert r.L.caro_drain_tuples_begin_q(*r.drain_args(), 1, q, None) == E_STATE
    assert r.L.caro_last_error().decode() == "caro_drain_tuples_begin_q" + BEFORE[2][1]
    assert r.L.caro_drain_tuples_begin_x(*r.drain_args(), 1, None, f, None) == E_STATE
    assert r.L.caro_last_error().decode() == "caro_drain_tuples_begin_x" + BEFORE[3][1]
    assert r.L.caro_drain_parked_begin_q(*r.drain_args(), q, None) == E_STATE
    assert r.L.caro_last_error().decode() == "caro_drain_parked_begin_q" + BEFORE[2][1]
    assert r.L.caro_drain_parked_begin_x(*r.drain_args(), None, f, None) == E_STATE
    assert r.L.caro_last_error().decode() == "caro_drain_parked_begin_x" + BEFORE[3][1]
    if which == "rig":
        r.cancel()
