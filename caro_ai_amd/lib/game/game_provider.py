"""`-g 0/1` game selection, as lib/game/game_provider.py:5-22 of the reference; `-g 2` (caro on 15 x 15, five to
win) goes beyond it."""
from caro_ai_amd.lib.game.caro import Caro
from caro_ai_amd.lib.game.connect_four import ConnectFour
from caro_ai_amd.lib.game.tictactoe import TicTacToe


def add_game_argument(parser):
    parser.add_argument("-g", "--game", required=True, choices=["0", "1", "2"],
                        help="The type of game. 0: Connect4, 1: TicTacToe, 2: Caro (15x15, blocked fives do not win)")


def get_game(args):
    if args.game == "2":
        return Caro(15, 5)
    return ConnectFour() if args.game == "0" else TicTacToe()
