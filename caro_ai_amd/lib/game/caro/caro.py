"""Caro: gomoku in which a five blocked at both ends by the opponent does not win -- the game this project is named
after, and an extension beyond the reference (whose TicTacToe is plain k-in-a-row).

Caro(n, k) is TicTacToe(n, k) in everything -- board, state int, codec, planes, action space, legality, draw,
render -- except the win test (the rule as stated in include/caro_hip.h): after the mover's stone, one of the four
lines through it holds a run of more than k of the mover's stones, or a run of exactly k whose two end cells are not
both opponent stones; a cell beyond the edge does not block.  The test lives in caro_rules.h (CaroRules), compiled
into the host helpers this class calls and into every tree and rule kernel the engine runs for it."""
from caro_ai_amd import _lib
from caro_ai_amd.lib.game.tictactoe.tictactoe import TicTacToe


class Caro(TicTacToe):
    kind = _lib.GAME_CARO

    def __init__(self, n: int = 15, k_to_win: int = 5):
        super().__init__(n, k_to_win)
