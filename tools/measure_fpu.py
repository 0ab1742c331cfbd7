#!/usr/bin/env python3
"""What first-play urgency reduction does on Connect4 with the shipped best_026_12000.dat: a match, and the width of
the search at the root.

The match: two lock-step engines, one per side, one with FPU (--reduction / --root-reduction) and one without.  Each ply
the mover's engine gets the position through set_roots (its tree is kept: it holds that side's own earlier searches),
searches at tau = 0, and its most visited move is applied on the host.  set_roots leaves an engine's ply counter where it
is, and these engines never step, so generated noise would repeat the rows of ply 0 at every move of a game; the tool
therefore hands every search explicit Dirichlet rows, drawn on the host from a generator seeded with (--seed, ply): fresh
at every ply, and the same for both colour assignments.  --games slots are played twice, once with the FPU engine as
player 0 and once as player 1: paired seeds, colours swapped.  Reported: wins / losses / draws of the FPU side and the
game count.
The width: self-play (lock-step, tau = 1 for the first 10 plies) with and without FPU; the mean number of distinct root
children visited per searched ply.

    python tools/measure_fpu.py [--games 256] [--searches 25] [--batch 8] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def _engine(game, hip, G, S, B, seed, sbt0, fpu):
    from caro_ai_amd.engine import SelfPlayEngine
    eng = SelfPlayEngine(game, G, evaluators=[hip], max_batch=B, steps_before_tau_0=sbt0, seed=seed, device="cuda:0",
                         searches_hint=S)
    if fpu is not None:
        eng.set_fpu(*fpu)
    return eng


def match(game, hip, G, S, B, seed, fpu, fpu_player):
    """G games, the FPU engine playing `fpu_player` -> (wins, losses, draws) of the FPU side"""
    from caro_ai_amd import config as cfg
    engs = {fpu_player: _engine(game, hip, G, S, B, seed, 0, fpu), 1 - fpu_player: _engine(game, hip, G, S, B, seed, 0, None)}
    states = [game.initial_state] * G
    live = np.ones(G, bool)
    res = [0, 0, 0]
    player = ply = 0
    A = game.action_space
    while live.any():
        eng = engs[player]
        eng.set_roots([s if ok else game.initial_state for s, ok in zip(states, live)], [player] * G)
        noise = np.random.default_rng([seed, ply]).dirichlet(np.full(A, cfg.ALPHA), size=(S, G, B))
        eng.search(S, B, noise=noise)
        _, counts = eng.policy()
        moves = counts.cpu().numpy().argmax(1)
        for g in np.flatnonzero(live):
            states[g], won = game.move(states[g], int(moves[g]), player)
            if won:
                res[0 if player == fpu_player else 1] += 1
                live[g] = False
            elif not game.possible_moves(states[g]):
                res[2] += 1
                live[g] = False
        player = 1 - player
        ply += 1
    over = [e.counters()["overflows"] for e in engs.values()]
    for e in engs.values():
        e.close()
    assert not any(over), "a tree overflowed"
    return res


def root_width(game, hip, G, S, B, seed, fpu, plies):
    """mean number of distinct root children visited per searched ply of self-play"""
    eng = _engine(game, hip, G, S, B, seed, 10, fpu)
    tot = n = 0
    live = np.ones(G, bool)
    for _ in range(plies):
        eng.search(S, B)
        _, counts = eng.policy()
        _, done, _ = eng.step()
        tot += int((counts.cpu().numpy()[live] > 0).sum())
        n += int(live.sum())
        live = done.cpu().numpy() == 0
        if not live.any():
            break
    assert eng.counters()["overflows"] == 0
    eng.close()
    return tot / max(n, 1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--games", type=int, default=256, help="slots per colour assignment (the match has twice as many games)")
    ap.add_argument("--searches", type=int, default=25)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reduction", type=float, default=0.5)
    ap.add_argument("--root-reduction", type=float, default=0.25)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--weights", default=os.path.join(ROOT, "tests", "golden", "weights", "best_026_12000.dat"))
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args(argv)
    from caro_ai_amd.lib.game.connect_four import ConnectFour
    from caro_ai_amd.lib.model import Net
    from caro_ai_amd.net_hip import HipNet
    game = ConnectFour()
    net = Net(game.obs_shape, game.action_space)
    net.load_state_dict(torch.load(args.weights, map_location="cpu"))
    hip = HipNet(net.to("cuda:0").eval(), "cuda:0")
    fpu = (args.reduction, args.root_reduction)
    G, S, B = args.games, args.searches, args.batch
    first = match(game, hip, G, S, B, args.seed, fpu, 0)
    second = match(game, hip, G, S, B, args.seed, fpu, 1)
    out = {"config": "connect four, %dx%d sims/move, tau = 0, %s, hip f32w net" % (S, B, os.path.basename(args.weights)),
           "reduction": fpu[0], "root_reduction": fpu[1], "games": 2 * G,
           "fpu_as_player0": dict(zip(("wins", "losses", "draws"), first)),
           "fpu_as_player1": dict(zip(("wins", "losses", "draws"), second)),
           "fpu_total": dict(zip(("wins", "losses", "draws"), [a + b for a, b in zip(first, second)])),
           "root_children_per_ply": {"off": root_width(game, hip, G, S, B, args.seed, None, 12),
                                     "fpu": root_width(game, hip, G, S, B, args.seed, fpu, 12)}}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return out


if __name__ == "__main__":
    main()
