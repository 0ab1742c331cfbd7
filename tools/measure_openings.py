#!/usr/bin/env python3
"""What random openings do to Connect4 self-play data: config 2's shape (1 024 games, 25 x 8 sims per move, the
staggered stream form -- every slot restarts in place -- with the shipped best_026_12000.dat on the fused HIP net), same
engine, warm-up and window as tools/measure_playout_cap.py.  Settings: max_plies = 0 (off, the baseline the others are
read against), 2, 4, 8.  Every setting gets an engine of its own, plays --warmup passes (one pass = `searches` launches)
and then times --steps passes.  Per setting: finished games/s, tuples/s, searched plies per game, opening plies per
game, the share of distinct (state, player) among the tuples of the window and among tuples 0 - 3 of each game, and the
result split (player 0 wins / loses / draws).  Whether such games train a better net is not measured here.

    python tools/measure_openings.py [--warmup 40] [--steps 80] > profiles/openings_measure.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from measure_playout_cap import window  # noqa: E402

SBT0 = 10
SETTINGS = [0, 2, 4, 8]


def distinct_share(states, players):
    """distinct (state, player) rows / rows"""
    if not len(players):
        return 0.0
    rows = np.concatenate([np.asarray(states).reshape(len(players), -1).astype(np.int64),
                           np.asarray(players).reshape(-1, 1).astype(np.int64)], axis=1)
    return len(np.unique(rows, axis=0)) / len(rows)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=40, help="passes before the timed window of each setting")
    ap.add_argument("--steps", type=int, default=80, help="passes in the timed window")
    ap.add_argument("--weights", default=os.path.join(ROOT, "caro_ai_amd", "data", "weights", "best_026_12000.dat"))
    args = ap.parse_args(argv)
    from caro_ai_amd.engine import SelfPlayEngine
    from caro_ai_amd.lib.game.connect_four import ConnectFour
    from caro_ai_amd.lib.model import Net
    from caro_ai_amd.net_hip import HipNet
    from caro_ai_amd.resign import split_games
    device, S, B, seed = "cuda:0", 25, 8, 0
    game = ConnectFour()
    net = Net(game.obs_shape, game.action_space)
    net.load_state_dict(torch.load(args.weights, map_location="cpu"))
    net = net.to(device).eval()
    hip = HipNet(net, device)
    rows = []
    for mp in SETTINGS:
        eng = SelfPlayEngine(game, args.games, evaluators=[hip], max_batch=B, steps_before_tau_0=SBT0, seed=seed,
                             device=device, searches_hint=S, stagger=True)
        eng.restart(seed=seed)
        eng.set_openings(mp)
        c, drains, dt = window(eng, S, B, args.warmup, args.steps)
        eng.close()
        host = [{k: v.cpu().numpy() for k, v in d.items()} for d in drains]
        games = [g for d in host for g in split_games(d)]
        n_tuples = sum(len(g["z"]) for g in games)
        head_s = np.concatenate([g["states"][:4] for g in games])
        head_p = np.concatenate([g["players"][:4] for g in games])
        res = np.array([g["result"] for g in games])
        row = {"max_plies": mp, "games": len(games), "tuples": n_tuples, "seconds": dt,
               "games_per_s": c["finished"] / dt, "tuples_per_s": n_tuples / dt, "plies_per_s": c["plies"] / dt,
               "plies_per_game": n_tuples / max(len(games), 1),
               "open_plies_per_game": float(np.mean([g["open"][0] for g in games])) if mp else 0.0,
               "distinct_share_window": distinct_share(np.concatenate([d["states"] for d in host]),
                                                       np.concatenate([d["players"] for d in host])),
               "distinct_share_tuples_0_3": distinct_share(head_s, head_p),
               "result_split": {"player0_wins": float((res == 1).mean()), "player0_loses": float((res == -1).mean()),
                                "draws": float((res == 0).mean())}}
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
    out = {"config": "connect four, %d games, %dx%d sims/move, staggered stream, %s, hip f32w net, steps_before_tau_0 %d"
                     % (args.games, S, B, os.path.basename(args.weights), SBT0),
           "warmup_passes": args.warmup, "steps": args.steps, "runs": rows}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
