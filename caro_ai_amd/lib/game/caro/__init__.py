"""`from caro_ai_amd.lib.game.caro import Caro`, as for the two games of the reference."""
from caro_ai_amd.lib.game.caro.caro import Caro  # noqa: F401
