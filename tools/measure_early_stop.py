#!/usr/bin/env python3
"""What the early stop of decided tau = 0 plies buys in Connect4 self-play: config 2's shape (1 024 games, 25 x 8 sims
per move, the staggered stream form -- every slot restarts in place -- with the shipped best_026_12000.dat on the fused
HIP net), same engine, warm-up and window as tools/measure_playout_cap.py.  Settings: off; min_minibatches = 24 (above
M - 2: recording only); 1; 8; the playout cap at (0.25, 5) alone; the cap with min_minibatches = 1.  Every setting
restarts the engine, plays --warmup passes (one pass = `searches` launches) and then times --steps passes.  Per
setting: plies/s, finished games/s, tuples/s (the training tuples of the finished games: all plies, full plies under
the cap), minibatches per ply and per tau = 0 ply, the share of tau = 0 plies cut, and -- from --sample single launches
after the window, each followed by caro_pending_leaves -- the mean and maximum net rows per launch and the share of
launches past one round of tiles (256 CUs x 6 boards = 1 536).

    python tools/measure_early_stop.py [--warmup 40] [--steps 80] [--sample 200]
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

from measure_playout_cap import ROUND_ROWS, launch_rows, window  # noqa: E402

SBT0 = 10
SETTINGS = [("off", None, None), ("record", None, 24), ("min1", None, 1), ("min8", None, 8),
            ("cap", (0.25, 5), None), ("cap+min1", (0.25, 5), 1)]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=40, help="passes before the timed window of each setting")
    ap.add_argument("--steps", type=int, default=80, help="passes in the timed window")
    ap.add_argument("--sample", type=int, default=200, help="single launches sampled for the net rows per launch")
    ap.add_argument("--weights", default=os.path.join(ROOT, "tests", "golden", "weights", "best_026_12000.dat"))
    args = ap.parse_args(argv)
    from caro_ai_amd import early_stop
    from caro_ai_amd.engine import SelfPlayEngine
    from caro_ai_amd.lib.game.connect_four import ConnectFour
    from caro_ai_amd.lib.model import Net
    from caro_ai_amd.net_hip import HipNet
    device, S, B, seed = "cuda:0", 25, 8, 0
    game = ConnectFour()
    net = Net(game.obs_shape, game.action_space)
    net.load_state_dict(torch.load(args.weights, map_location="cpu"))
    net = net.to(device).eval()
    hip = HipNet(net, device)
    rows = []
    for name, cap, floor in SETTINGS:
        # (neither feature can be switched off again: every setting gets an engine of its own, restarted)
        eng = SelfPlayEngine(game, args.games, evaluators=[hip], max_batch=B, steps_before_tau_0=SBT0, seed=seed,
                             device=device, searches_hint=S, stagger=True)
        eng.restart(seed=seed)
        if cap is not None:
            eng.set_playout_cap(*cap)
        if floor is not None:
            eng.set_early_stop(floor)
        c, drains, dt = window(eng, S, B, args.warmup, args.steps)
        n_tuples = sum(int(d["z"].shape[0]) for d in drains)
        n_train = sum(int(d["full"].sum()) for d in drains) if cap is not None else n_tuples
        row = {"setting": name, "playout_cap": cap, "min_minibatches": floor,
               "plies_per_s": c["plies"] / dt, "games_per_s": c["finished"] / dt, "tuples_per_s": n_train / dt,
               "minibatches_per_ply": c["sims"] / B / max(c["plies"], 1)}
        if floor is not None:
            host = [{k: d[k].cpu().numpy() for k in ("games", "mb", "full") if k in d} for d in drains]
            st = early_stop.stop_stats(host, S, SBT0, cap[1] if cap is not None else None)
            tau0 = np.concatenate([early_stop.ply_indices(d["games"]) >= SBT0 for d in host])
            mb = np.concatenate([d["mb"] for d in host]).astype(np.int64)
            row.update(st, tau0_share=float(tau0.mean()), minibatches_per_tau0_ply=float(mb[tau0].mean()),
                       tau0_plies_cut_share=st["stop_plies"] / max(st["stop_tau0_plies"], 1))
        sample = launch_rows(eng, B, args.sample)
        row.update(net_rows_per_launch=sum(sample) / len(sample), net_rows_max=max(sample),
                   launches_past_one_round=sum(r > ROUND_ROWS for r in sample) / len(sample), seconds=dt)
        eng.close()
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
    by = {r["setting"]: r for r in rows}
    keys = ("plies_per_s", "games_per_s", "tuples_per_s", "minibatches_per_ply")
    out = {"config": "connect four, %d games, %dx%d sims/move, staggered stream, %s, hip f32w net, steps_before_tau_0 %d"
                     % (args.games, S, B, os.path.basename(args.weights), SBT0),
           "warmup_passes": args.warmup, "steps": args.steps, "sampled_launches": args.sample, "runs": rows,
           "vs_off": {r["setting"]: {k: r[k] / by["off"][k] for k in keys} for r in rows},
           "cap+min1_vs_cap": {k: by["cap+min1"][k] / by["cap"][k] for k in keys}}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
