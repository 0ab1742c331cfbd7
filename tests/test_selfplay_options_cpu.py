"""caro_ai_amd.selfplay_options: the record train.self_play, train.self_play_stream and train.fit build from their eight
option keywords, and the engine calls it makes.  The engine is a fake that records its calls; the expected sequences
are written out here as train.py made them before the record existed (one `if X is not None: eng.set_X(...)` per
option, in this order; on a reused stream the first three always, the other five only when changed, behind one flush)."""
import pytest

from caro_ai_amd import train
from caro_ai_amd.lib.game.connect_four import ConnectFour
from caro_ai_amd.selfplay_options import NAMES, SelfPlayOptions

GAME = ConnectFour()
ALL = dict(resign=(-0.9, 0.25), playout_cap=(0.5, 2), early_stop=1, openings=3, forced_playouts=2, fpu=(0.5, 0.25),
           virtual_loss=2, temperature=(1, 0.25, True))
ALWAYS = [("set_resign", (-0.9, 0.25)), ("set_playout_cap", (0.5, 2)), ("set_early_stop", (1,))]
DRAIN = object()


class FakeEngine:
    """the eight attributes at None, a flush() that hands out DRAIN, set_* that record (name, args) and keep the value"""

    def __init__(self, **have):
        self.calls = []
        for name in ("resign", "playout_cap", "early_stop", "openings", "forced_playouts", "fpu", "virtual_loss",
                     "temperature"):
            setattr(self, name, have.get(name))

    def flush(self):
        self.calls.append(("flush", ()))
        return DRAIN

    def _set(self, name, args, value):
        self.calls.append(("set_" + name, args))
        setattr(self, name, value)

    def set_resign(self, *a):
        self._set("resign", a, a)

    def set_playout_cap(self, *a):
        self._set("playout_cap", a, a)

    def set_early_stop(self, *a):
        self._set("early_stop", a, a[0])

    def set_openings(self, *a):
        self._set("openings", a, a[0])

    def set_forced_playouts(self, *a):
        self._set("forced_playouts", a, a[0])

    def set_fpu(self, *a):
        self._set("fpu", a, a)

    def set_virtual_loss(self, *a):
        self._set("virtual_loss", a, a[0])

    def set_temperature(self, *a):
        self._set("temperature", a, a)


def test_the_table_is_the_eight_options_in_the_order_they_are_applied():
    assert NAMES == ("resign", "playout_cap", "early_stop", "openings", "forced_playouts", "fpu", "virtual_loss",
                     "temperature")
    assert SelfPlayOptions._fields == NAMES


def test_apply_with_all_eight_on_makes_the_eight_set_calls_in_order_and_no_flush():
    opts = SelfPlayOptions.of(GAME, **ALL)
    eng = FakeEngine()
    assert opts.apply(eng) is None
    assert eng.calls == ALWAYS + [("set_openings", (3,)), ("set_forced_playouts", (2.0,)), ("set_fpu", (0.5, 0.25)),
                                  ("set_virtual_loss", (2,)), ("set_temperature", (1.0, 0.25, True))]
    assert opts.key() == (True,) * 8
    assert opts.kwargs() == dict(ALL, forced_playouts=2.0, temperature=(1.0, 0.25, True))
    assert SelfPlayOptions.of(GAME, **opts.kwargs()) == opts  # (what fit hands on is taken as it is)
    assert SelfPlayOptions.of(GAME, *ALL.values()) == opts  # (the values in table order)


def test_nothing_on_makes_no_call():
    opts = SelfPlayOptions.of(GAME)
    eng = FakeEngine()
    opts.apply(eng)
    assert opts.reapply(eng) is None
    assert eng.calls == [] and opts.key() == (False,) * 8 and opts == SelfPlayOptions()


@pytest.mark.parametrize("kw", [dict(openings=0), dict(forced_playouts=0), dict(fpu=0), dict(fpu=(0, 0)),
                                dict(virtual_loss=0), dict(temperature=(1, 0, False))])
def test_the_off_values_fold_to_the_all_off_record(kw):
    assert SelfPlayOptions.of(GAME, **kw) == SelfPlayOptions()


def test_values_are_normalised_once():
    assert SelfPlayOptions.of(GAME, fpu=0.5).fpu == (0.5, 0.5)
    opts = SelfPlayOptions.of(GAME, resign=(-1, 1), playout_cap=(1, 2.0), early_stop=True)
    assert opts.resign == (-1.0, 1.0) and opts.playout_cap == (1.0, 2) and opts.early_stop == 1
    assert [type(x) for x in opts.resign + opts.playout_cap + (opts.early_stop,)] == [float, float, float, int, int]
    assert opts.key() == (True, True, True, False, False, False, False, False)


@pytest.mark.parametrize("kw", [dict(openings=42), dict(openings=65), dict(openings=1.0), dict(forced_playouts=65),
                                dict(virtual_loss=17), dict(virtual_loss=1.0), dict(virtual_loss=True), dict(fpu=2.5),
                                dict(fpu=(0.5, 0.5, 0.5)), dict(fpu="x"), dict(temperature=(0.01, 0, False)),
                                dict(temperature=(1, 9, False)), dict(temperature=(1, 0, 2))])
def test_bad_values_raise_value_error(kw):
    with pytest.raises(ValueError):
        SelfPlayOptions.of(GAME, **kw)


def test_an_unknown_option_is_a_type_error():
    with pytest.raises(TypeError):
        SelfPlayOptions.of(GAME, virtual_los=2)


def test_reapply_on_an_engine_that_has_the_values_calls_the_three_always_setters_only():
    opts = SelfPlayOptions.of(GAME, **ALL)
    eng = FakeEngine(**opts.kwargs())
    assert opts.reapply(eng) is None
    assert eng.calls == ALWAYS


def test_reapply_flushes_once_before_the_first_changed_option():
    opts = SelfPlayOptions.of(GAME, **ALL)
    eng = FakeEngine(**dict(opts.kwargs(), forced_playouts=1.0, temperature=(1.0, 0.5, True)))
    assert opts.reapply(eng) is DRAIN
    assert eng.calls == ALWAYS + [("flush", ()), ("set_forced_playouts", (2.0,)), ("set_temperature", (1.0, 0.25, True))]


def test_reapply_with_only_openings_changed_flushes_right_before_set_openings():
    opts = SelfPlayOptions.of(GAME, **ALL)
    eng = FakeEngine(**dict(opts.kwargs(), openings=5))
    assert opts.reapply(eng) is DRAIN
    assert eng.calls == ALWAYS + [("flush", ()), ("set_openings", (3,))]


def test_reapply_leaves_alone_what_is_off():
    opts = SelfPlayOptions.of(GAME, early_stop=2, fpu=0.25)
    eng = FakeEngine(early_stop=2, openings=4, fpu=(0.5, 0.5))
    assert opts.reapply(eng) is DRAIN
    assert eng.calls == [("set_early_stop", (2,)), ("flush", ()), ("set_fpu", (0.25, 0.25))] and eng.openings == 4


def test_streamed_self_play_has_every_setter_and_property():
    from caro_ai_amd.engine import SelfPlayEngine, StreamedSelfPlay
    for name in ("resign", "playout_cap", "early_stop", "openings", "forced_playouts", "fpu", "virtual_loss",
                 "temperature"):
        prop, setter = vars(StreamedSelfPlay)[name], vars(StreamedSelfPlay)["set_" + name]
        assert isinstance(prop, property) and prop.__doc__ and prop.fset is None
        assert callable(setter) and setter.__name__ == "set_" + name and setter.__doc__.strip()
        assert callable(vars(SelfPlayEngine)["set_" + name]) and vars(SelfPlayEngine)["set_" + name].__doc__.strip()


def test_options_from_args_with_every_flag_is_the_record_of_the_keywords():
    argv = ["-n", "x", "-g", "0", "--resign-threshold", "-0.9", "--resign-playthrough", "0.25", "--playout-cap-full",
            "0.5", "--playout-cap-fast", "2", "--early-stop", "--opening-plies", "3", "--forced-playouts", "2",
            "--fpu-reduction", "0.5", "--fpu-root-reduction", "0.25", "--virtual-loss", "2", "--tau-early", "1",
            "--tau-late", "0.25", "--visit-targets"]
    assert train.options_from_args(train.parse_args(argv), GAME) == SelfPlayOptions.of(GAME, **ALL)
    assert train.options_from_args(train.parse_args(argv[:4]), GAME) == SelfPlayOptions()
    zeros = argv[:4] + ["--opening-plies", "0", "--forced-playouts", "0", "--fpu-reduction", "0", "--virtual-loss", "0",
                        "--tau-early", "1"]
    assert train.options_from_args(train.parse_args(zeros), GAME) == SelfPlayOptions()


def test_a_bad_command_line_is_rejected_at_its_first_bad_option():
    base = ["-n", "x", "-g", "0"]
    bad = [(["--resign-target-fp", "0.05"], "--resign-target-fp needs"), (["--resign-threshold", "2"], "--resign-threshold"),
           (["--playout-cap-fast", "2"], "--playout-cap-fast needs"), (["--early-stop", "0"], "--early-stop MIN"),
           (["--opening-plies", "42"], "--opening-plies N"), (["--forced-playouts", "65"], "--forced-playouts K"),
           (["--fpu-root-reduction", "0.5"], "--fpu-root-reduction needs"), (["--virtual-loss", "17"], "--virtual-loss N"),
           (["--tau-late", "9"], "--tau-early T")]
    for i, (flags, text) in enumerate(bad):
        with pytest.raises(SystemExit, match=text):
            train.options_from_args(train.parse_args(base + flags), GAME)
        if i >= 2:  # (with every later mistake on the line as well: the first one wins)
            later = [f for fl, _ in bad[i + 1:] for f in fl]
            with pytest.raises(SystemExit, match=text):
                train.options_from_args(train.parse_args(base + later + flags), GAME)
    with pytest.raises(SystemExit, match="--resign-threshold must"):
        train.options_from_args(train.parse_args(base + ["--resign-threshold", "2", "--playout-cap-fast", "2"]), GAME)
