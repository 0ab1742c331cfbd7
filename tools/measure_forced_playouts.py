#!/usr/bin/env python3
"""What forced playouts and policy target pruning cost and change in Connect4 self-play: config 2's shape (1 024 games,
25 x 8 sims per move, the staggered stream form -- every slot restarts in place -- with the shipped best_026_12000.dat on
the fused HIP net) played with the feature off, at k = 2 (KataGo's value), under the playout cap (0.25, 5) alone, and under
the cap with k = 2.  Every setting gets its own engine, plays --warmup passes (one pass = `searches` launches) and then
times --steps passes.  Per setting: plies/s, training tuples/s (tuples of the finished games; under the cap those of full
plies), the forced share of the root descents made under the rule, the visits pruned per simulation, and the mean entropy
(nats) of the training tuples' pi at tau = 1 plies -- the off rows are the targets before the feature, the k = 2 rows the
pruned targets of the forced search.

    python tools/measure_forced_playouts.py [--warmup 40] [--steps 80]
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

SBT0 = 10


def tau1_entropy(drains):
    """mean entropy of pi over the training tuples of tau = 1 plies (a game's first SBT0 plies), and their number"""
    from caro_ai_amd import forced_playouts as fp
    from caro_ai_amd.resign import split_games
    hs = []
    for d in drains:
        for g in split_games({k: v.cpu().numpy() for k, v in d.items()}):
            pi = g["pi"][:SBT0]
            if "full" in g:
                pi = pi[g["full"][:SBT0].astype(bool)]
            hs.append(fp.entropy(pi))
    hs = np.concatenate(hs) if hs else np.zeros(0)
    return (float(hs.mean()) if len(hs) else 0.0), int(len(hs))


def main(argv=None):
    from measure_playout_cap import window
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=40, help="passes before the timed window of each setting")
    ap.add_argument("--steps", type=int, default=80, help="passes in the timed window")
    ap.add_argument("--weights", default=os.path.join(ROOT, "tests", "golden", "weights", "best_026_12000.dat"))
    ap.add_argument("--out", default=None, help="also write the table to this JSON file")
    args = ap.parse_args(argv)
    from caro_ai_amd import forced_playouts as fp
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
    for k, cap in ((None, None), (2.0, None), (None, (0.25, 5)), (2.0, (0.25, 5))):
        eng = SelfPlayEngine(game, args.games, evaluators=[hip], max_batch=B, steps_before_tau_0=SBT0, seed=seed,
                             device=device, searches_hint=S, stagger=True)
        if cap is not None:
            eng.set_playout_cap(*cap)
        if k is not None:
            eng.set_forced_playouts(k)
        for _ in range(args.warmup):
            eng.move(S, B)
        eng.flush()
        s0 = fp.stats(eng)
        c, drains, dt = window(eng, S, B, 0, args.steps)
        s1 = fp.stats(eng)
        st = {n: s1[n] - s0[n] for n in fp.STAT_NAMES}
        n_tuples = sum(int(d["z"].shape[0]) for d in drains)
        n_train = sum(int(d["full"].sum()) for d in drains) if cap is not None else n_tuples
        h, n_h = tau1_entropy(drains)
        row = {"k": k, "p_full": None if cap is None else cap[0], "fast": None if cap is None else cap[1],
               "plies_per_s": c["plies"] / dt, "tuples_per_s": n_train / dt, "sims_per_ply": c["sims"] / max(c["plies"], 1),
               "forced_share": st["forced_descents"] / st["root_descents"] if st["root_descents"] else 0.0,
               "pruned_visits_share": st["visits_removed"] / max(c["sims"], 1),
               "pruned_plies_share": st["pruned_plies"] / max(c["plies"], 1),
               "pi_entropy_tau1": h, "tau1_tuples": n_h, "seconds": dt}
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
        eng.close()
    out = {"config": "connect four, %d games, %dx%d sims/move, staggered stream, %s, hip f32w net"
                     % (args.games, S, B, os.path.basename(args.weights)),
           "warmup_passes": args.warmup, "steps": args.steps, "runs": rows,
           "vs_off": [{n: r[n] / rows[0][n] for n in ("plies_per_s", "tuples_per_s")} for r in rows]}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return out


if __name__ == "__main__":
    main()
