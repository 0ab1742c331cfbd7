#!/usr/bin/env python3
"""Golden vectors for caro (blocked-five gomoku), by RUNNING THE REFERENCE's search (build container only; the
outputs are committed, the reference is not).  The reference has no caro game: it is stated here as a subclass of the
reference's own `TicTacToe` whose `move` applies the caro rule, written in plain Python from the rule text
(include/caro_hip.h) -- runs along each line, no bit tricks, nothing of the product.  The search, the
game loop and the harness are the reference's `MCTS` / `play_game` under make_golden.py's harness (table net,
table-driven noise and move choice).

  rules_caro.json.gz   random transitions on 5x5 k4, 7x7 k4, 9x9 k5, 15x15 k5: state, move, player, next state,
                       caro-won, gomoku-won (the reference's check_win).  Moves are drawn uniformly, except that a
                       move which completes a blocked run of exactly k (gomoku would end the game, caro does not)
                       is taken with probability 1/2 when one exists, so that such transitions are plentiful.
  synth_caro.json.gz   whole table-net games on 7x7 k4 (3 x 8 sims), 9x9 k5 and 15x15 k5 (25 x 8), one 15x15
                       game at 50 x 8, tau = 1 throughout.  The uids are the lowest of a candidate range whose games
                       contain a ply where the gomoku rule would have ended the game and caro did not;
                       `gomoku_plies` lists those plies (the last ply is not looked at).  Such games are rare under
                       a search (it takes an open win first): tests/golden/CARO.md says how many were found.

Usage:  python tests/golden/make_golden_caro.py
"""
import multiprocessing as mp
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (puts the reference on sys.path and imports its lib)
from lib.game.tictactoe import tictactoe_helpers as ref_helpers  # noqa: E402

LINES = (ref_helpers.get_row, ref_helpers.get_col, ref_helpers.get_diag, ref_helpers.get_antidiag)


def line_wins_caro(line, k, me):
    """the rule, run by run: a run longer than k wins; a run of exactly k wins unless the cells just before and
    just after it are both on the board and both hold the opponent's stones"""
    n, i = len(line), 0
    while i < n:
        if line[i] != me:
            i += 1
            continue
        j = i
        while j < n and line[j] == me:
            j += 1
        run = j - i
        if run > k:
            return True
        if run == k:
            before = i > 0 and line[i - 1] == 1 - me
            after = j < n and line[j] == 1 - me
            if not (before and after):
                return True
        i = j
    return False


def caro_won(board, coord, k, me):
    return any(line_wins_caro(f(board, coord), k, me) for f in LINES)


class CaroRef(mg.TicTacToe):
    """the reference's TicTacToe with the caro win test"""

    def move(self, mcts_state, move, player):
        assert player == self.player_white or player == self.player_black
        assert move >= 0 and move <= self.action_space
        board = self.convert_mcts_state_to_list_state(mcts_state)
        r, c = divmod(move, self.board_len)
        board[r][c] = player
        return self.encode_game_state(board), caro_won(board, (r, c), self.k_to_win, player)


def both_rules(game, state, move, player):
    board = game.convert_mcts_state_to_list_state(state)
    r, c = divmod(move, game.board_len)
    board[r][c] = player
    return (game.encode_game_state(board), caro_won(board, (r, c), game.k_to_win, player),
            ref_helpers.check_win(board, (r, c), game.k_to_win, player))


# ------------------------------------------------------------------ rules_caro
def rules_vectors(n, k, n_diff, n_plain, rng):
    game = CaroRef(n, k)
    recs, diff, plain = [], 0, 0
    tries = 0
    while (diff < n_diff or plain < n_plain) and tries < 400:
        tries += 1
        s, p = game.initial_state, int(rng.integers(2))
        while True:
            legal = game.possible_moves(s)
            if not legal:
                break
            outs = {m: both_rules(game, s, m, p) for m in legal}
            special = [m for m in legal if outs[m][2] and not outs[m][1]]
            if special and rng.random() < 0.5:
                mv = special[int(rng.integers(len(special)))]
            else:
                mv = int(legal[int(rng.integers(len(legal)))])
            s2, cw, gw = outs[mv]
            assert (s2, cw) == game.move(s, mv, p)
            if cw != gw and diff < n_diff:
                recs.append({"s": str(s), "m": int(mv), "p": p, "s2": str(s2), "caro": bool(cw), "gomoku": bool(gw)})
                diff += 1
            elif cw == gw and plain < n_plain:
                recs.append({"s": str(s), "m": int(mv), "p": p, "s2": str(s2), "caro": bool(cw), "gomoku": bool(gw)})
                plain += 1
            s, p = s2, 1 - p
            if cw:
                break
    return recs, diff


# ------------------------------------------------------------------ synth_caro
def synth_eval_fast(planes, A):
    """make_golden.synth_eval, vectorised (uint64 arithmetic wraps as the masked Python ints do)"""
    L = planes.shape[0]
    flat = (planes.reshape(L, -1) != 0).astype(np.uint64)
    D = flat.shape[1]
    coef = np.array([mg.mix64(0x5851f42d4c957f2d + j) | 1 for j in range(D)], dtype=np.uint64)

    def mix(z):
        z = z ^ (z >> np.uint64(30))
        z = z * np.uint64(0xbf58476d1ce4e5b9)
        z = z ^ (z >> np.uint64(27))
        z = z * np.uint64(0x94d049bb133111eb)
        return z ^ (z >> np.uint64(31))

    h = (flat * coef).sum(axis=1, dtype=np.uint64)
    steps = np.arange(1, A + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    ha = mix(h[:, None] + steps[None, :])
    P = (((ha >> np.uint64(20)) & np.uint64(1023)) + np.uint64(1)).astype(np.float32) / np.float32(8192.0)
    hv = mix(h ^ np.uint64(0xA5A5A5A5A5A5A5A5))
    v = ((hv >> np.uint64(20)) % np.uint64(2001)).astype(np.int64) - 1000
    return P, v.astype(np.float32) / np.float32(1024.0)


class FastSynthNet(mg.SynthNet):
    def forward(self, x):
        P, v = synth_eval_fast(x.numpy(), self.A)
        return torch.from_numpy(P), torch.from_numpy(v).reshape(-1, 1)


def gomoku_plies(game, g):
    """plies (before the last) whose move the gomoku rule would have called a win: the game went on under caro"""
    out = []
    for i in range(g["plies"] - 1):
        a = str(g["states"][i]).rjust(game.board_len ** 2, "0")
        b = str(g["states"][i + 1]).rjust(game.board_len ** 2, "0")
        cells = [j for j in range(len(a)) if a[j] != b[j]]
        assert len(cells) == 1
        _, cw, gw = both_rules(game, int(g["states"][i]), cells[0], g["players"][i])
        assert not cw
        if gw:
            out.append(i)
    return out


def play_one(job):
    n, k, S, B, sbt0, seed, uid = job
    torch.set_num_threads(1)
    game = CaroRef(n, k)
    net = FastSynthNet(game)
    t0 = time.time()
    g = mg.strip(mg.play_reference(game, net, net, 1, sbt0, S, B, uid & 1, seed, uid, True), False)
    g["n"], g["k"] = n, k
    g["gomoku_plies"] = gomoku_plies(game, g)
    print("  %dx%d k%d %dx%d uid %d: %d plies, result %d, %d nodes, blocked-win plies %s, %.0f s"
          % (n, n, k, S, B, uid, g["plies"], g["result"], g["trace"][-1]["nodes"], g["gomoku_plies"],
             time.time() - t0), flush=True)
    return g


# (n, k, searches, batch, steps before tau 0, seed, first uid, candidates at most, games kept).  tau = 1 for the whole
# game: a blocked five needs long, loose games; with tau = 0 the table-net search takes the first open five it sees.
SYNTH = [(7, 4, 3, 8, 49, 61, 8000, 800, 4),
         (9, 5, 25, 8, 81, 67, 8100, 60, 2),
         (15, 5, 25, 8, 225, 71, 8200, 21, 2),
         (15, 5, 50, 8, 225, 73, 8300, 7, 1)]


def main():
    t0 = time.time()
    rng = np.random.default_rng(20261015)
    x = (rng.random((64, 2, 9, 9)) < 0.3).astype(np.float32)
    P1, v1 = mg.synth_eval(x, 81)
    P2, v2 = synth_eval_fast(x, 81)
    assert np.array_equal(P1, P2) and np.array_equal(v1, v2)

    boards = []
    total_diff = 0
    for n, k, n_diff, n_plain in [(5, 4, 0, 300), (7, 4, 80, 300), (9, 5, 80, 300), (15, 5, 80, 200)]:
        recs, diff = rules_vectors(n, k, n_diff, n_plain, rng)
        total_diff += diff
        boards.append({"n": n, "k": k, "recs": recs})
        print("rules %dx%d k%d: %d transitions, %d where caro and gomoku differ" % (n, n, k, len(recs), diff))
    assert total_diff >= 200
    mg.dump("rules_caro.json.gz", {"kind": "caro", "boards": boards})

    # candidates in uid order; the first `keep` games with a blocked-win ply are kept (imap keeps the order, so the
    # choice does not depend on timing)
    games, hit = [], 0
    for n, k, S, B, sbt0, seed, uid0, cand, keep in SYNTH:
        chosen, plain = [], []
        with mp.get_context("fork").Pool(max(1, min(7, (os.cpu_count() or 2) - 1))) as pool:
            for g in pool.imap(play_one, [(n, k, S, B, sbt0, seed, uid0 + i) for i in range(cand)], chunksize=1):
                (chosen if g["gomoku_plies"] else plain).append(g)
                if len(chosen) == keep:
                    break
        hit += len(chosen)
        games += chosen + plain[:keep - len(chosen)]
        print("%dx%d k%d %dx%d: kept uids %s (%.0f s)" % (n, n, k, S, B, [g["uid"] for g in games[-keep:]],
                                                        time.time() - t0), flush=True)
    if 2 * hit < len(games):
        print("only %d of %d games hold a blocked-win ply" % (hit, len(games)))
    mg.dump("synth_caro.json.gz", {"kind": "caro", "games": games})
    print("%d games, %d with a blocked-win ply; done in %.1fs" % (len(games), hit, time.time() - t0))


if __name__ == "__main__":
    main()
