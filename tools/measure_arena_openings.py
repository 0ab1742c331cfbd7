#!/usr/bin/env python3
"""How independent the games of an arena match are, with and without paired openings: the shipped Connect4
checkpoints best_025_10600.dat (net1) vs best_026_12000.dat, train.evaluate's 20 x 16 sims per move, tau = 0 from move
0, one tree per player, the opener alternating with the uid.  Two matches of --games games under the same seed: all
from the empty board, and as pairs from random openings of up to --opening-plies plies
(SelfPlayEngine.set_openings(..., paired=True)).  Per match: the number of distinct games (distinct sequences of tuple
states), the score of net1, the standard errors over games and over pairs, the pairs the opening decided, and the wall
time of the match (engine built, games played and drained).  Data, not thresholds.

    python tools/measure_arena_openings.py [--games 64] [--opening-plies 4] [--seed 0]

prints the JSON and writes it to profiles/arena_openings_measure.json.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

S, B = 20, 16


def match(game, net1, net2, n_games, seed, opening_plies, device):
    """the games of uids 0 .. n_games - 1, one slot each (lib.utils.play_games' engine) -> per-game dicts by uid, seconds"""
    from caro_ai_amd.engine import SelfPlayEngine, staggered_geometry
    from caro_ai_amd.resign import split_games
    torch.cuda.synchronize()
    t0 = time.time()
    stagger = staggered_geometry(game, B, False)
    eng = SelfPlayEngine(game, n_games, net1=net1, net2=net2, n_stores=2, max_batch=B, steps_before_tau_0=0, seed=seed,
                         uid_base=0, first_player_mode=2, device=device, searches_hint=S, stagger=stagger,
                         stagger_recycle=False, games_limit=n_games)
    games = {}
    try:
        if opening_plies:
            eng.set_openings(opening_plies, paired=True)
        for _ in range(42 * S + 64):
            eng.search(S, B)
            eng.step()
            d = eng.drain(recycle=not stagger)
            if int(d["games"].shape[0]):
                for g in split_games({k: v.cpu().numpy() for k, v in d.items()}):
                    games[g["uid"]] = g
            if len(games) == n_games:
                break
        assert len(games) == n_games and eng.counters()["overflows"] == 0
    finally:
        eng.close()
    torch.cuda.synchronize()
    return games, time.time() - t0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--games", type=int, default=64)
    ap.add_argument("--opening-plies", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "arena_openings_measure.json"))
    args = ap.parse_args(argv)
    from caro_ai_amd import match_stats
    from caro_ai_amd.lib.game.connect_four import ConnectFour
    from caro_ai_amd.play import load_checkpoint
    device = "cuda:0"
    game = ConnectFour()
    weights = os.path.join(ROOT, "caro_ai_amd", "data", "weights")
    names = ("best_025_10600.dat", "best_026_12000.dat")
    net1, net2 = (load_checkpoint(game, os.path.join(weights, n), device) for n in names)
    match(game, net1, net2, 2, args.seed, 0, device)  # (the first engine of a process pays for the library and the nets)
    rows = []
    for plies in (0, args.opening_plies):
        games, dt = match(game, net1, net2, args.games, args.seed, plies, device)
        results = [games[u]["result"] for u in sorted(games)]
        lines = {np.ascontiguousarray(games[u]["states"]).tobytes() for u in games}
        paired = match_stats.summary(match_stats.pair_table(results))
        row = {"opening_plies": plies, "games": len(results), "distinct_games": len(lines),
               "score": paired["score"], "ratio": paired["ratio"], "wins": paired["wins"], "losses": paired["losses"],
               "draws": paired["draws"], "se_games": paired["se_games"], "se_pairs": paired["se_pairs"],
               "split_pairs": paired["split_pairs"], "pairs": paired["pairs"], "seconds": dt,
               "plies_per_game": float(np.mean([len(games[u]["z"]) for u in games])),
               "open_plies_per_game": float(np.mean([games[u]["open"][0] for u in games])) if plies else 0.0}
        if not plies:  # (from the empty board consecutive uids are no pair: the pair figures are there for comparison only)
            row["note"] = "unpaired match: se_pairs and split_pairs group consecutive uids, which share nothing"
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
    out = {"config": "connect four, %s (net1) vs %s, %d games, %dx%d sims/move, tau 0, one slot per game, seed %d"
                     % (names[0], names[1], args.games, S, B, args.seed), "runs": rows}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


if __name__ == "__main__":
    main()
