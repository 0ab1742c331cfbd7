"""The opt-in self-play options as ONE record: what train.self_play, train.self_play_stream and train.fit take as eight
keywords, checked once, and the only statement of how they reach an engine (SelfPlayEngine or StreamedSelfPlay).  A new
option is one row of TABLE; nothing here needs a GPU."""
import collections

from caro_ai_amd import forced_playouts as fp
from caro_ai_amd import fpu as fpu_mod
from caro_ai_amd import openings as op
from caro_ai_amd import temperature as temp_mod
from caro_ai_amd import virtual_loss as vl_mod


def _fpu(v, cells):
    pair = fpu_mod.check_pair(v)  # (r alone: the reduction of the root level too)
    return pair if pair != (0.0, 0.0) else None


def _temperature(v, cells):
    triple = temp_mod.check_triple(*v)
    return triple if temp_mod.is_on(triple) else None


# One row per option, in the order the engine is told about them:
#   name       the keyword of train's entry points = the engine's attribute; the engine's setter is set_<name>
#   splat      the setter takes the value's parts (set_resign(*v)) or the value whole (set_early_stop(v))
#   flush      a CHANGED value on a running stream needs the pending drain taken first (the engine refuses the set call
#              with a drain open); False: the setter is simply called again at every call of the stream
#   normalise  (value that is not None, the board's cell count) -> None (off) or the checked canonical value
TABLE = (
    ("resign", True, False, lambda v, cells: (float(v[0]), float(v[1]))),
    ("playout_cap", True, False, lambda v, cells: (float(v[0]), int(v[1]))),
    ("early_stop", False, False, lambda v, cells: int(v)),
    ("openings", False, True, lambda v, cells: op.limit(v, cells) or None),
    ("forced_playouts", False, True, lambda v, cells: fp.check_k(v) or None),
    ("fpu", True, True, _fpu),
    ("virtual_loss", False, True, lambda v, cells: vl_mod.check_n(v) or None),
    ("temperature", True, True, _temperature),
)
NAMES = tuple(row[0] for row in TABLE)


def _set(eng, name, splat, v):
    getattr(eng, "set_" + name)(*(v if splat else (v,)))


class SelfPlayOptions(collections.namedtuple("SelfPlayOptions", NAMES, defaults=(None,) * len(NAMES))):
    """the eight options, each None (off) or its checked value; immutable (a new threshold: `_replace(resign=...)`)"""
    __slots__ = ()

    @classmethod
    def of(cls, game, *values, **kw):
        """from what a caller passed (the eight keywords, or the values in TABLE order) and the game: "0 means off" is
        folded and every value checked (ValueError) here, once"""
        cells = game.obs_shape[1] * game.obs_shape[2]
        return cls(*(None if v is None else row[3](v, cells) for row, v in zip(TABLE, cls(*values, **kw))))

    def key(self):
        """which options are on: what an engine-cache key appends (an engine that records root Q, ply classes, ... is
        kept apart from one that does not)"""
        return tuple(v is not None for v in self)

    def kwargs(self):
        """the record as the keywords of train's entry points"""
        return self._asdict()

    def apply(self, eng):
        """every option that is on, on an engine that has played nothing yet: a fresh or a restarted one (the settings
        survive a restart; a restart opened its games under the kept setting and a new one re-opens them)"""
        for (name, splat, _, _), v in zip(TABLE, self):
            if v is not None:
                _set(eng, name, splat, v)

    def reapply(self, eng):
        """the same on a stream that goes on running: a flush-option only if its value changed, with the pending drain
        taken before the first such set call.  Returns that drain (its rows belong to this call) or None"""
        carried = None
        for (name, splat, flush, _), v in zip(TABLE, self):
            if v is None or (flush and getattr(eng, name) == v):
                continue
            if flush and carried is None:
                carried = eng.flush()
            _set(eng, name, splat, v)
        return carried
