#!/usr/bin/env python3
"""What virtual loss does at the headline shape -- Connect4, 1 024 games, 25 x 8, staggered, best_026_12000.dat -- for
n_vl in {0, 1, 2, 3}: throughput, batch diversity, launch times; and a match of n_vl = 2 against off.

Per n_vl: a staggered engine as bench.py runs it, --warmup moves, then --steps timed moves.  Recorded: plies/s and
node-expansions/s on the wall clock; expansions per simulation and the dropped share (descents dropped as duplicates of
a leaf of their own minibatch / simulations); the tree and the net launch time (sampled HIP events, caro_profile_read);
then --launch-samples single launches with the leaves of each read back: net rows per launch, mean and max.

The match: two lock-step engines, one per side, one with n_vl = 2 and one without, at equal simulations.  Each ply the
mover's engine gets the position through set_roots (its tree is kept), searches at tau = 0, and its most visited move is
applied on the host.  set_roots leaves an engine's ply counter where it is, and these engines never step, so generated
noise would repeat the rows of ply 0 at every move of a game; the tool therefore hands every search explicit Dirichlet
rows, drawn on the host from a generator seeded with (--seed, ply): fresh at every ply, and the same for both colour
assignments (tools/measure_fpu.py).  --games slots are played twice, colours swapped.

    python tools/measure_virtual_loss.py [--out profiles/virtual_loss_measure.json]
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


def throughput(game, hip, G, S, B, seed, n_vl, warmup, steps, samples):
    from caro_ai_amd import _lib
    from caro_ai_amd.engine import SelfPlayEngine, _ptr
    eng = SelfPlayEngine(game, G, evaluators=[hip], max_batch=B, seed=seed, device="cuda:0", searches_hint=S, stagger=True)
    eng.set_virtual_loss(n_vl)
    eng.profile(True)
    for _ in range(warmup):
        eng.move(S, B)
    eng.flush()
    torch.cuda.synchronize()
    c0 = eng.counters()
    eng.profile_read(reset=True)
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.move(S, B)
    eng.flush()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    c1 = eng.counters()
    prof = eng.profile_read(reset=True)
    eng.profile(False)
    d = {k: c1[k] - c0[k] for k in c1}
    rows = []
    for _ in range(samples):  # one launch at a time: the leaves it selected are the net launch's rows
        _lib.check(eng.L.caro_search_staggered(eng.h, hip.h, None, 1, B, _ptr(eng.planes), _ptr(eng.leaf_keys),
                                               _ptr(eng._probs), _ptr(eng._values), eng._stream()))
        rows.append(eng.pending_leaves())
    over = eng.counters()["overflows"]
    eng.close()
    assert over == 0, "a tree overflowed"
    us = {k: 1e3 * prof[k][0] / max(prof[k][1], 1) for k in ("select", "net")}
    return {"n_vl": n_vl, "plies_per_s": d["plies"] / dt, "expansions_per_s": d["expansions"] / dt,
            "expansions_per_sim": d["expansions"] / max(d["sims"], 1), "dropped_share": d["dropped"] / max(d["sims"], 1),
            "terminal_share": d["terminals"] / max(d["sims"], 1), "net_rows_per_launch_mean": float(np.mean(rows)),
            "net_rows_per_launch_max": int(np.max(rows)), "tree_launch_us": us["select"], "net_launch_us": us["net"],
            "timed_launches": (prof["select"][1], prof["net"][1])}


def match(game, hip, G, S, B, seed, n_vl, vl_player):
    """G games, the virtual-loss engine playing `vl_player` -> (wins, losses, draws) of that side"""
    from caro_ai_amd import config as cfg
    from caro_ai_amd.engine import SelfPlayEngine
    engs = {}
    for side in (0, 1):
        engs[side] = SelfPlayEngine(game, G, evaluators=[hip], max_batch=B, steps_before_tau_0=0, seed=seed,
                                    device="cuda:0", searches_hint=S)
    engs[vl_player].set_virtual_loss(n_vl)
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
                res[0 if player == vl_player else 1] += 1
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--concurrent", type=int, default=1024)
    ap.add_argument("--searches", type=int, default=25)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--launch-samples", type=int, default=50)
    ap.add_argument("--games", type=int, default=256, help="match slots per colour assignment (twice as many games)")
    ap.add_argument("--match-n", type=int, default=2, help="n_vl of the match's virtual-loss side")
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
    G, S, B = args.concurrent, args.searches, args.batch
    throughput(game, hip, 64, S, B, args.seed, 2, 2, 2, 2)  # first-use costs
    rows = [throughput(game, hip, G, S, B, args.seed, n, args.warmup, args.steps, args.launch_samples)
            for n in (0, 1, 2, 3)]
    out = {"config": "connect four, %d games, %dx%d sims/move, staggered, %s, hip f32w net; %d timed moves after %d"
                     % (G, S, B, os.path.basename(args.weights), args.steps, args.warmup),
           "throughput": rows}
    if args.games > 0:
        first = match(game, hip, args.games, S, B, args.seed, args.match_n, 0)
        second = match(game, hip, args.games, S, B, args.seed, args.match_n, 1)
        out["match"] = {"config": "tau = 0, n_vl = %d against off at %dx%d sims/move, %d games, colours swapped"
                                  % (args.match_n, S, B, 2 * args.games),
                        "vl_as_player0": dict(zip(("wins", "losses", "draws"), first)),
                        "vl_as_player1": dict(zip(("wins", "losses", "draws"), second)),
                        "vl_total": dict(zip(("wins", "losses", "draws"), [a + b for a, b in zip(first, second)]))}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return out


if __name__ == "__main__":
    main()
