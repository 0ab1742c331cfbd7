"""Hand-written search trees for the position-analysis tests: dicts state -> node row, small enough to follow by eye.
The CPU test checks the reference walker (tests/analysis_ref.py) on them; the GPU test pokes the same rows into an engine
and compares caro_principal_lines with the walker.  Every stored word is exact in float32 and tells its edge apart."""
import numpy as np


def row(A, visits):
    """a node row from {action: N}: W, Q, P and the strong flag are functions of (action, N), all float32-exact"""
    N = np.zeros(A, np.int32)
    W = np.zeros(A, np.float64)
    Q = np.zeros(A, np.float64)
    P = np.array([(a + 1) / 512.0 for a in range(A)], np.float32)
    strong = np.zeros(A, np.int32)
    for a, n in visits.items():
        N[a] = n
        W[a] = n * 0.25 - a * 0.125
        Q[a] = 0.5 - a / 16.0 - n / 64.0
        strong[a] = (a + n) & 1
    return {"N": N, "W": W, "Q": Q, "P": P, "W_is_f32": strong}


def play(game, state, player, moves):
    """the position after `moves`, sides alternating from `player`; no move of the sequence may end the game"""
    for mv in moves:
        state, won = game.move(state, mv, player)
        assert not won
        player = 1 - player
    return state


def ttt_tree(game):
    """TicTacToe(3, 3).  -> (nodes, roots): roots["open"] = (initial position, 1 to move), roots["late"] = a position two
    moves from a full board with 0 to move, roots["absent"] = a position that is no node.
    From "open" (root visits 5 + 3 + 3 + 1 = 12; ranking 4, 0, 8, 2: actions 0 and 8 tie at 3 visits):
      4 0 ...      after [4] actions 0 and 1 tie at 2: the line takes 0; [4, 0] is a node without visits: LEAF, len 2
      0 3 1 4 2    the top row: the fifth move WINS (depth 5: WIN, not DEPTH; depth 4: DEPTH)
      8            [8] is no node: LEAF, len 1
      2            [2] is a node whose edges have no visit: LEAF, len 1
    From "late": 6 8 fills the board without a line of three: DRAW, len 2; 8 alone: LEAF."""
    A, init = 9, game.initial_state
    nodes = {
        init: row(A, {4: 5, 0: 3, 8: 3, 2: 1}),
        play(game, init, 1, [4]): row(A, {0: 2, 1: 2, 5: 1}),
        play(game, init, 1, [4, 0]): row(A, {}),
        play(game, init, 1, [0]): row(A, {3: 4, 4: 1}),
        play(game, init, 1, [0, 3]): row(A, {1: 3}),
        play(game, init, 1, [0, 3, 1]): row(A, {4: 2, 8: 1}),
        play(game, init, 1, [0, 3, 1, 4]): row(A, {2: 1, 5: 1}),  # a tie at 1 visit: 2, the winning move
        play(game, init, 1, [2]): row(A, {}),
    }
    # X (1): 0 2 3 7, O (0): 1 4 5, O to move; 6 then 8 fill the board, nobody has three in a line
    late = init
    for mv, who in ((0, 1), (1, 0), (2, 1), (4, 0), (3, 1), (5, 0), (7, 1)):
        late, won = game.move(late, mv, who)
        assert not won
    nodes[late] = row(A, {6: 2, 8: 1})
    nodes[play(game, late, 0, [6])] = row(A, {8: 1})
    absent = play(game, init, 1, [1, 7])
    assert absent not in nodes
    return nodes, {"open": (init, 1), "late": (late, 0), "absent": (absent, 1)}


def c4_tree(game):
    """ConnectFour.  Root: the initial position, 1 to move; root visits 4 + 4 + 1 = 9; ranking 0, 3, 6 (0 and 3 tie).
      0 1 0 1 0 1 0   four of player 1 in column 0: the seventh move WINS (depth 7: WIN)
      3 3             after [3] actions 3 and 4 tie at 2: the line takes 3; [3, 3] is no node: LEAF, len 2
      6               [6] is no node: LEAF, len 1"""
    A, init = 7, game.initial_state
    nodes = {init: row(A, {3: 4, 0: 4, 6: 1})}
    line = [0, 1, 0, 1, 0, 1]
    for i in range(1, len(line) + 1):
        nodes[play(game, init, 1, line[:i])] = row(A, {line[i] if i < len(line) else 0: 7 - i, 5: 1})
    nodes[play(game, init, 1, [3])] = row(A, {4: 2, 3: 2})
    absent = play(game, init, 1, [2, 2])
    return nodes, {"open": (init, 1), "absent": (absent, 1)}
