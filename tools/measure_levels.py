#!/usr/bin/env python3
"""What session levels cost, what mixed budgets save, and how strong a few levels play: Connect4, the shipped nets, 256
sessions, the bot's 40 x 8 simulations per move.

    python tools/measure_levels.py [--parent DIR] [--alternations 3] [--reps 7] [--games 64] [--out FILE]

(a) COST.  One `move_bots` call for 256 mid-game sessions, all at the pool's own strength, in three forms: the checkout
    of the parent commit in DIR (built, with its libcaro_hip.so; skipped without --parent), this tree with no level ever
    named ("none": the engine is never told of levels), and this tree with every session at Level(40, 0.0, 0) ("same":
    levels on, saying nothing).  Each form runs in a process of its own, the forms alternate, and each run reports the
    median of `reps` timed rounds as tools/measure_session_pool.py takes it; the figure of a form is the median of its
    runs, and the spread of a form's runs is what a difference has to be read against.
(b) GAIN.  The same call with the sessions at 10 / 20 / 40 minibatches in equal thirds ("mixed") against "same".
(c) STRENGTH.  `games` games per level of a pool with levels against a second pool's full-strength bot (40 x 8, tau 0,
    best_026_12000.dat) that moves as the "human"; the level's bot moves first in every other game.  Score = (wins +
    draws / 2) / games.  Data, not a claim: one seed, one opponent.
One JSON document on stdout (and in --out)."""
import argparse
import json
import os
import random
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
W26 = os.path.join("caro_ai_amd", "data", "weights", "best_026_12000.dat")
W25 = os.path.join("caro_ai_amd", "data", "weights", "best_025_10600.dat")
SESSIONS, SCRIPTED_ROUNDS = 256, 3


def worker(tree, form, reps):
    """one form of (a) / (b) in this process, on the package of `tree`: {"ms_median", "ms_min", "ms_max"}"""
    sys.path.insert(0, tree)
    import torch
    from caro_ai_amd.lib.game.connect_four import ConnectFour
    from caro_ai_amd.lib import session_pool as sp
    game = ConnectFour()
    pool = sp.SessionPool(game, os.path.join(tree, W26), slots=SESSIONS, device="cuda:0", seed=7)
    rng = random.Random(1256)

    def level_of(i):
        if form == "none":
            return {}
        return {"level": sp.Level(40 if form == "same" else (10, 20, 40)[i % 3], 0.0, 0)}

    opened = [0]

    def new():
        opened[0] += 1
        return pool.open(True, **level_of(opened[0]))

    def fresh(n):
        ss = [new() for _ in range(n)]
        for _ in range(SCRIPTED_ROUNDS):  # (three plies by each side never end a connect four game)
            for s in ss:
                s.move_player(rng.choice(game.possible_moves(s.state)))
            pool.move_bots(ss)
        return ss

    sessions = fresh(SESSIONS)
    times = []
    for _ in range(reps + 1):  # (the first rep pays first-use costs and is dropped)
        while True:
            for s in sessions:
                if not s.finished and not s.bots_turn():
                    s.move_player(rng.choice(game.possible_moves(s.state)))
            ended = [s for s in sessions if s.finished]
            if not ended:
                break
            for s in ended:
                pool.close(s)
            sessions = [s for s in sessions if not s.finished] + fresh(len(ended))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pool.move_bots(sessions)
        times.append(time.perf_counter() - t0)
    assert pool.engine.counters()["overflows"] == 0
    pool.close_pool()
    t = np.array(times[1:]) * 1e3
    print(json.dumps({"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max())}))


def strength(games):
    sys.path.insert(0, ROOT)
    from caro_ai_amd.lib.game.connect_four import ConnectFour
    from caro_ai_amd.lib.session_pool import Level, SessionPool
    game = ConnectFour()
    levels = [Level(40, 0.0, 0), Level(20, 0.0, 0), Level(10, 0.0, 0), Level(2, 0.0, 0), Level(40, 1.0, 0),
              Level(40, 0.0, 1)]
    n = games * len(levels)
    mine = SessionPool(game, [os.path.join(ROOT, W26), os.path.join(ROOT, W25)], slots=n, device="cuda:0", seed=7)
    full = SessionPool(game, os.path.join(ROOT, W26), slots=n, device="cuda:0", seed=8)
    pairs = []  # (the level's session, the opponent's session in which the level's bot is the human)
    for i in range(n):
        first = i % 2 == 0  # the level's bot moves first
        pairs.append((mine.open(not first, level=levels[i // games]), full.open(first)))
    score = [0.0] * len(levels)
    plies = [0] * len(levels)
    for _ in range(43):
        for me, pool in ((0, mine), (1, full)):
            ready = [p for p in pairs if p[me].bots_turn()]
            for p, (move, _, won) in zip(ready, pool.move_bots([p[me] for p in ready])):
                if not p[1 - me].finished:
                    p[1 - me].move_player(move)
                k = pairs.index(p) // games
                plies[k] += 1
                if won:
                    score[k] += 1.0 if me == 0 else 0.0
                elif p[me].finished:
                    score[k] += 0.5
        if all(a.finished for a, _ in pairs):
            break
    assert all(a.finished and b.finished for a, b in pairs)
    assert mine.engine.counters()["overflows"] == 0 and full.engine.counters()["overflows"] == 0
    mine.close_pool()
    full.close_pool()
    return [{"level": {"searches": lv.searches, "tau": lv.tau, "net": os.path.basename((W26, W25)[lv.net])},
             "games": games, "score": score[k] / games, "plies_per_game": plies[k] / games} for k, lv in enumerate(levels)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--games", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", nargs=2, metavar=("TREE", "FORM"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(os.path.abspath(args.worker[0]), args.worker[1], args.reps)
    forms = ([("parent", os.path.abspath(args.parent), "none")] if args.parent else []) + [
        ("none", ROOT, "none"), ("same", ROOT, "same"), ("mixed", ROOT, "mixed")]
    runs = {name: [] for name, _, _ in forms}
    for _ in range(args.alternations):
        for name, tree, form in forms:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--worker", tree, form],
                                 cwd=tree, check=True, capture_output=True, text=True, timeout=300).stdout
            runs[name].append(json.loads(out.strip().splitlines()[-1]))
    cost = {}
    for name, rs in runs.items():
        med = [r["ms_median"] for r in rs]
        cost[name] = {"ms": float(np.median(med)), "runs_ms": med, "spread_ms": float(max(med) - min(med)),
                      "rounds_min_max_ms": [min(r["ms_min"] for r in rs), max(r["ms_max"] for r in rs)]}
    import torch
    out = {"what": "one SessionPool.move_bots call for 256 mid-game connect four sessions, best_026_12000.dat, 40 x 8 "
                   "simulations per move unless a level says otherwise; wall ms up to host-visible results",
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "alternations": args.alternations,
           "forms": {"parent": "the parent commit", "none": "this tree, no level ever named",
                     "same": "every session at Level(40, 0.0, 0)", "mixed": "budgets 10 / 20 / 40 in equal thirds"},
           "cost": cost, "strength_vs_full_40x8": strength(args.games),
           "command": "python tools/measure_levels.py%s --alternations %d --reps %d --games %d"
                      % (" --parent DIR" if args.parent else "", args.alternations, args.reps, args.games)}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
