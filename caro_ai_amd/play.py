#!/usr/bin/env python3
"""Round-robin arena between checkpoints: the command-line surface of the reference's play.py:15-76 (same
arguments, same pairing rule, same printed lines) on the batched HIP engine.

Every ordered pair (first, second) of the given checkpoints meets `--rounds` times: tau = 0 from the first move,
PLAY_MCTS_SEARCHES x PLAY_MCTS_BATCH_SIZE simulations per move, a fresh pair of trees per game, the opening side
alternating with the game id (the reference draws it at random, play.py:47-52 / utils.py:65-66).  All rounds of
a pairing advance together on the GPU; with several ranks (torchrun) each rank plays a contiguous share of the
rounds and the win / loss / draw counts are all-reduced.

    python -m caro_ai_amd.play -g 0 --cuda a.dat b.dat -r 64

--opening-plies N (an extension beyond the reference, off by default): the rounds of a pairing are played as pairs from
random openings of up to N plies -- rounds 2j and 2j + 1 start from colour-swapped twins of one opening, so each net
plays it once from each side -- and a second line per pairing carries the match statistics (caro_ai_amd.match_stats:
score, pairs, their standard error, Elo with its 95 % interval).  `--rounds` must then be even.
"""
import argparse
import itertools
import sys
import time
from dataclasses import dataclass

import numpy as np
import torch

from caro_ai_amd import config as cfg
from caro_ai_amd import match_stats, parallel
from caro_ai_amd.lib import model, utils
from caro_ai_amd.lib.game import game_provider


@dataclass(frozen=True)
class Tally:
    wins: int = 0
    losses: int = 0
    draws: int = 0

    @classmethod
    def of(cls, net1_results):
        return cls(sum(r > 0 for r in net1_results), sum(r < 0 for r in net1_results),
                   sum(r == 0 for r in net1_results))

    def as_tuple(self):
        return (self.wins, self.losses, self.draws)

    def mirrored(self):
        """the same games seen from the other side of the board"""
        return (self.losses, self.wins, self.draws)

    def __str__(self):
        return "w=%d, l=%d, d=%d" % self.as_tuple()


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("models", nargs="+", help="The list of models (at least 2) to play against each other")
    ap.add_argument("-r", "--rounds", type=int, default=2, help="Count of rounds to perform for every pair")
    ap.add_argument("--cuda", default=False, action="store_true", help="Enable CUDA")
    ap.add_argument("--seed", type=int, default=0, help="key of the generated noise / move uniforms")
    ap.add_argument("--node-cap", type=int, default=0,
                    help="nodes per tree (default: searches x batch x cells, which cannot overflow; an overflow ends the run)")
    ap.add_argument("--opening-plies", type=int, default=None, metavar="N",
                    help="play the rounds of every pairing as pairs from random openings of up to N plies, each opening "
                         "twice with the colours swapped, and print the match statistics (default: off; 0 = off; "
                         "--rounds must be even)")
    game_provider.add_game_argument(ap)
    args = ap.parse_args(argv)
    if args.opening_plies is not None:
        from caro_ai_amd import openings
        game = game_provider.get_game(args)
        try:
            args.opening_plies = openings.limit(args.opening_plies, game.obs_shape[1] * game.obs_shape[2]) or None
        except ValueError as e:
            ap.error("--opening-plies N must be in [0, %d] and below the board's cell count: %s" % (openings.MAX_PLIES, e))
        if args.opening_plies is not None and args.rounds & 1:
            ap.error("--opening-plies plays the rounds as pairs: --rounds must be even, got %d" % args.rounds)
    return args


def load_checkpoint(game, path, device):
    """a `.dat` file is torch.save(net.state_dict()) (train.py:214-216); the net is built with the checkpoint's own
    depth (`train.py --res-blocks`), so checkpoints of different depths meet without a flag -- the two nets of a pair
    launch may differ in depth"""
    weights = torch.load(path, map_location=lambda storage, loc: storage)
    return model.Net.from_state_dict(weights, game.obs_shape, game.action_space).to(device).eval()


def meet(game, first, second, rounds, seed, uid_base, device, node_cap=None, opening_plies=None):
    """`rounds` games `first` (player 0) vs `second`; this rank plays its share, every rank gets the total.
    opening_plies: the rounds as pairs from random openings (even `rounds` and `uid_base`; the ranks share whole pairs);
    returns (tally, the match's 3 x 3 match_stats.pair_table) then."""
    rank, _, world = parallel.env_rank() if parallel.is_dist() else (0, 0, 1)
    if opening_plies is not None:
        lo, n = parallel.shard_rounds(rounds // 2, rank, world)
        lo, n = 2 * lo, 2 * n
        mine = []
        if n:
            mine = utils.play_games(game, n, None, first, second, steps_before_tau_0=0,
                                    mcts_searches=cfg.PLAY_MCTS_SEARCHES, mcts_batch_size=cfg.PLAY_MCTS_BATCH_SIZE,
                                    concurrent=min(n, 1024), seed=seed, uid_base=uid_base + lo, device=device,
                                    first_player_mode=2, node_cap=node_cap, openings=opening_plies, opening_pairs=True)
        flat = parallel.allreduce_counts(match_stats.pair_table(mine).reshape(-1).tolist(), device)
        table = np.asarray(flat, dtype=np.int64).reshape(3, 3)
        s = match_stats.summary(table)
        return Tally(s["wins"], s["losses"], s["draws"]), table
    lo, n = parallel.shard_rounds(rounds, rank, world)
    mine = []
    if n:
        mine = utils.play_games(game, n, None, first, second, steps_before_tau_0=0,
                                mcts_searches=cfg.PLAY_MCTS_SEARCHES, mcts_batch_size=cfg.PLAY_MCTS_BATCH_SIZE,
                                concurrent=min(n, 1024), seed=seed, uid_base=uid_base + lo, device=device,
                                first_player_mode=2, node_cap=node_cap)
    return Tally(*parallel.allreduce_counts(Tally.of(mine).as_tuple(), device))


def main(argv=None):
    args = parse_args(argv)
    rank, local_rank, world = parallel.init()
    device = parallel.local_device(local_rank) if world > 1 else "cuda:0"  # the engine is GPU only; --cuda is accepted as is
    game = game_provider.get_game(args)
    agents = [(path, load_checkpoint(game, path, device)) for path in args.models]

    per_agent, per_pair = {}, {}
    say = print if rank == 0 else (lambda *a, **k: None)
    pairings = list(itertools.permutations(range(len(agents)), 2))  # every ordered pair, first index outermost
    for k, (i, j) in enumerate(pairings):
        (name_i, net_i), (name_j, net_j) = agents[i], agents[j]
        started = time.time()
        table = None
        if args.opening_plies is not None:
            tally, table = meet(game, net_i, net_j, args.rounds, args.seed, k * args.rounds, device,
                                args.node_cap or None, args.opening_plies)
        else:
            tally = meet(game, net_i, net_j, args.rounds, args.seed, k * args.rounds, device, args.node_cap or None)
        say("%s vs %s -> %s" % (name_i, name_j, tally))
        if table is not None:
            say(match_stats.text(match_stats.summary(table)))
        if rank == 0:
            sys.stderr.write("Speed %.2f games/s\n" % (args.rounds / (time.time() - started)))
        sys.stdout.flush()
        utils.update_counts(per_agent, name_i, tally.as_tuple())
        utils.update_counts(per_agent, name_j, tally.mirrored())
        utils.update_counts(per_pair, (name_i, name_j), tally.as_tuple())

    say("Leaderboard:")
    for name, (w, l, d) in sorted(per_agent.items(), key=lambda item: item[1][0], reverse=True):  # by total wins
        say("%s: \t w=%d, l=%d, d=%d" % (name, w, l, d))
    return per_agent, per_pair


if __name__ == "__main__":
    main()
