#!/usr/bin/env python3
"""What resignation saves in Connect4 self-play: config 2's shape (1 024 games, 25 x 8 sims per move, the staggered
stream form -- every slot restarts in place -- with the shipped best_026_12000.dat on the fused HIP net) played with
resignation off (recording root Q only, threshold -1) and at three thresholds taken from the off run's root-Q
quantiles, playthrough share 0.1.  Every setting restarts the engine, plays --warmup passes (one pass = one ply per
game on average) and then times --steps passes.  Per setting: finished games/s, tuples/s, mean plies per game, resigned
share and the false-positive rate over the playthrough games that finished in the timed window.

    python tools/measure_resign.py [--warmup 80] [--steps 160] [--quantiles 0.02,0.05,0.10]
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


def window(eng, S, B, warmup, steps, seed, playthrough):
    from caro_ai_amd.resign import split_games
    for _ in range(warmup):
        eng.move(S, B)
    eng.flush()
    torch.cuda.synchronize()
    c0 = eng.counters()
    t0 = time.perf_counter()
    drains = []
    for _ in range(steps):
        d = eng.move(S, B)
        if d is not None and d["games"].shape[0]:
            drains.append(d)
    d = eng.flush()
    if d is not None and d["games"].shape[0]:
        drains.append(d)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    c1 = eng.counters()
    if c1["overflows"] != c0["overflows"]:
        raise RuntimeError("the node pool overflowed")
    games = [g for d in drains for g in split_games({k: v.cpu() for k, v in d.items()}, seed, playthrough)]
    return games, dt


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=80, help="passes before the timed window of each setting")
    ap.add_argument("--steps", type=int, default=160, help="passes in the timed window")
    ap.add_argument("--quantiles", default="0.02,0.05,0.10", help="root-Q quantiles of the off run used as thresholds")
    ap.add_argument("--playthrough", type=float, default=0.1)
    ap.add_argument("--weights", default=os.path.join(ROOT, "tests", "golden", "weights", "best_026_12000.dat"))
    args = ap.parse_args(argv)
    from caro_ai_amd.engine import SelfPlayEngine
    from caro_ai_amd.lib.game.connect_four import ConnectFour
    from caro_ai_amd.lib.model import Net
    from caro_ai_amd.net_hip import HipNet
    from caro_ai_amd.resign import false_positive_rate
    device, S, B, seed = "cuda:0", 25, 8, 0
    game = ConnectFour()
    net = Net(game.obs_shape, game.action_space)
    net.load_state_dict(torch.load(args.weights, map_location="cpu"))
    net = net.to(device).eval()
    eng = SelfPlayEngine(game, args.games, evaluators=[HipNet(net, device)], max_batch=B, steps_before_tau_0=10,
                         seed=seed, device=device, searches_hint=S, stagger=True)
    rows = []

    def run(t):
        eng.restart(seed=seed)
        eng.set_resign(t, args.playthrough)
        games, dt = window(eng, S, B, args.warmup, args.steps, seed, args.playthrough)
        n = len(games)
        tuples = sum(len(g["z"]) for g in games)
        pt = [g for g in games if g["playthrough"]]
        row = {"threshold": t, "games": n, "games_per_s": n / dt, "tuples_per_s": tuples / dt,
               "mean_plies": tuples / max(n, 1), "resigned_share": sum(g["resigned"] for g in games) / max(n, 1),
               "playthrough_games": len(pt), "false_positive": false_positive_rate(games, t),
               "playthrough_triggered": sum(bool((g["q"] < t).any()) for g in pt), "seconds": dt}
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
        return games

    off = run(-1.0)
    qs = np.concatenate([g["q"] for g in off])
    thresholds = [float(np.quantile(qs, float(x))) for x in args.quantiles.split(",")]
    for t in thresholds:
        run(t)
    eng.close()
    base = rows[0]
    out = {"config": "connect four, %d games, %dx%d sims/move, staggered stream, %s, hip f32w net, playthrough %.2f"
                     % (args.games, S, B, os.path.basename(args.weights), args.playthrough),
           "warmup_passes": args.warmup, "steps": args.steps, "quantiles": args.quantiles, "runs": rows,
           "games_per_s_vs_off": [r["games_per_s"] / base["games_per_s"] for r in rows]}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
