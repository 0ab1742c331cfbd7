#!/usr/bin/env python3
"""What the temperature triple does to the tuples at the headline shape -- Connect4, 1 024 games, 25 x 8, staggered,
best_026_12000.dat -- for off, (1, 0, visit targets) and (1, 0.25, visit targets); and what the feature costs.

Per setting: a staggered engine as bench.py runs it (slots restart at once), --warmup moves, then --steps timed moves
whose drains are kept on the device and read after the clock stops.  Recorded over the games that finished in the timed
window: onehot_share (tuples whose pi has a single non-zero entry / tuples), the mean entropy of the tuples' pi (nats),
the mean game length (tuples per game), the distinct positions among the games' last searched plies (and their share of
the games), and plies/s on the wall clock.  The setting "off, full form" is the engine without the feature held in the
full form of the one-wave tree kernels (set_kernel_form(1)): the kernels a setting with the feature on runs, so the
plies/s of (1, 0, visit targets) against it is the cost of the feature itself.

    python tools/measure_temperature.py [--out profiles/temperature_measure.json]
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


def run(game, hip, G, S, B, seed, triple, full_form, warmup, steps):
    from caro_ai_amd.engine import SelfPlayEngine
    from caro_ai_amd import temperature as tp
    eng = SelfPlayEngine(game, G, evaluators=[hip], max_batch=B, seed=seed, device="cuda:0", searches_hint=S, stagger=True)
    if full_form:
        eng.set_kernel_form(1)
    if triple is not None:
        eng.set_temperature(*triple)
    form = eng.kernel_form()
    for _ in range(warmup):
        eng.move(S, B)
    eng.flush()
    torch.cuda.synchronize()
    c0 = eng.counters()
    drains = []
    t0 = time.perf_counter()
    for _ in range(steps):
        d = eng.move(S, B)
        if d is not None:
            drains.append(d)
    d = eng.flush()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if d is not None:
        drains.append(d)
    c1 = eng.counters()
    eng.close()
    assert c1["overflows"] == 0, "a tree overflowed"
    drains = [x for x in drains if int(x["games"].shape[0])]
    if not drains:  # (a window too short for any game to finish)
        return {"setting": str(triple), "games": 0, "plies_per_s": (c1["plies"] - c0["plies"]) / dt}
    pi = torch.cat([x["pi"] for x in drains]).cpu().numpy()
    recs = torch.cat([x["games"] for x in drains]).cpu().numpy().reshape(-1, 4)
    states = torch.cat([x["states"] for x in drains]).cpu().numpy()
    counts = recs[:, 3].astype(np.int64) + 1  # a game has steps + 1 tuples, its last ply first
    assert int(counts.sum()) == len(pi)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    last = {states[i].tobytes() for i in first.tolist()}
    with np.errstate(divide="ignore", invalid="ignore"):
        ent = -np.where(pi > 0, pi * np.log(pi), 0.0).sum(axis=1)
    return {"setting": "off" if triple is None else "tau_early %g, tau_late %g, visit_targets %s" % triple,
            "kernel_form": "full" if form else "lean", "games": int(len(recs)), "tuples": int(len(pi)),
            "onehot_share": tp.onehot_share(pi), "pi_entropy_mean": float(ent.mean()),
            "game_length_mean": float(counts.mean()), "distinct_last_positions": len(last),
            "distinct_last_positions_share": len(last) / max(len(recs), 1),
            "plies_per_s": (c1["plies"] - c0["plies"]) / dt}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--concurrent", type=int, default=1024)
    ap.add_argument("--searches", type=int, default=25)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=3, help="timed runs per setting, interleaved (plies/s of each is kept)")
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
    run(game, hip, 64, S, B, args.seed, (1.0, 0.25, True), False, 2, 2)  # first-use costs
    settings = [(None, False), (None, True), ((1.0, 0.0, True), False), ((1.0, 0.25, True), False)]
    rows = [None] * len(settings)
    for _ in range(max(1, args.repeats)):  # interleaved: a drift of the box hits every setting alike
        for i, (triple, full) in enumerate(settings):
            r = run(game, hip, G, S, B, args.seed, triple, full, args.warmup, args.steps)
            if rows[i] is None:
                rows[i] = dict(r, plies_per_s_runs=[])
            rows[i]["plies_per_s_runs"].append(r["plies_per_s"])
    for r in rows:
        r["plies_per_s"] = float(np.mean(r["plies_per_s_runs"]))
    out = {"config": "connect four, %d games, %dx%d sims/move, staggered, %s, hip f32w net; %d timed moves after %d, "
                     "%d runs per setting" % (G, S, B, os.path.basename(args.weights), args.steps, args.warmup,
                                              max(1, args.repeats)),
           "settings": rows}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return out


if __name__ == "__main__":
    main()
