#!/usr/bin/env python3
"""What the caro win test costs on the GPU: config 4's shape (1 024 games, 15 x 15, k = 5, 50 x 8 sims per move,
eviction with a 4 096-node cap, the fused HIP net with seed-0 weights, lock-step as bench.py's config-4 leg) for
gomoku (TicTacToe(15, 5)) and caro (Caro(15, 5)) in one process.  Both engines are first played to mid-game
(--warmup moves each), then timed windows of --steps moves alternate gomoku / caro --rounds times.  Reports
node-expansions/s and the tree kernel's HIP-event time per move (the `select` slot of the fused form; the engine
times a sample of the launches, the same sample for both games) of each, and caro / gomoku ratios of the medians.

    python tools/measure_caro.py [--warmup 40] [--steps 8] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def make(game, G, S, B, device):
    from caro_ai_amd.engine import SelfPlayEngine
    from caro_ai_amd.lib.model import Net
    from caro_ai_amd.net_hip import HipNet
    torch.manual_seed(0)
    net = Net(game.obs_shape, game.action_space).to(device).eval()
    return SelfPlayEngine(game, G, evaluators=[HipNet(net, device, mode="f32w")], max_batch=B, steps_before_tau_0=10,
                          seed=0, device=device, searches_hint=S, node_cap=4096, evict=True)


def window(eng, S, B, steps):
    torch.cuda.synchronize()
    c0 = eng.counters()
    eng.profile_read(reset=True)
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.search(S, B)
        eng.step()
        eng.drain(recycle=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    c1 = eng.counters()
    prof = eng.profile_read(reset=True)
    if c1["overflows"] != c0["overflows"]:
        raise RuntimeError("the node pool overflowed")
    return {"expansions_per_s": (c1["expansions"] - c0["expansions"]) / dt,
            "tree_ms_per_move": prof["select"][0] / steps, "net_ms_per_move": prof["net"][0] / steps,
            "finished": c1["finished"] - c0["finished"]}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=40, help="moves played before the first timed window")
    ap.add_argument("--steps", type=int, default=8, help="moves per timed window")
    ap.add_argument("--rounds", type=int, default=3, help="gomoku / caro window pairs")
    args = ap.parse_args(argv)
    from caro_ai_amd.lib.game.caro import Caro
    from caro_ai_amd.lib.game.tictactoe import TicTacToe
    device, S, B = "cuda:0", 50, 8
    engines = {"gomoku": make(TicTacToe(15, 5), args.games, S, B, device),
               "caro": make(Caro(15, 5), args.games, S, B, device)}
    for name, eng in engines.items():
        eng.profile(True)
        window(eng, S, B, args.warmup)
    runs = {name: [] for name in engines}
    for r in range(args.rounds):
        for name, eng in engines.items():
            runs[name].append(window(eng, S, B, args.steps))
            print("round %d %-6s %s" % (r, name, json.dumps({k: round(v, 3) for k, v in runs[name][-1].items()})),
                  file=sys.stderr, flush=True)
    for eng in engines.values():
        eng.close()
    med = {name: {k: float(np.median([x[k] for x in rs])) for k in ("expansions_per_s", "tree_ms_per_move",
                                                                    "net_ms_per_move")} for name, rs in runs.items()}
    out = {"config": "1024 games, 15x15 k=5, 50x8 sims/move, eviction (4096 nodes), hip f32w net, lock-step",
           "warmup_moves": args.warmup, "steps": args.steps, "rounds": args.rounds, "median": med,
           "runs": runs,
           "caro_vs_gomoku": {"expansions_per_s": med["caro"]["expansions_per_s"] / med["gomoku"]["expansions_per_s"],
                              "tree_ms_per_move": med["caro"]["tree_ms_per_move"] / med["gomoku"]["tree_ms_per_move"]}}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
