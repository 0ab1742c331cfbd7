#!/usr/bin/env python3
"""`SessionPool.analyse(searches=0)` against the same read-out walked from the host over `SelfPlayEngine.lookup`, the
only way to get it before caro_principal_lines: Connect4, shipped best_026_12000.dat, 256 sessions a few plies deep,
top = 3, depth = 8.

    python tools/measure_analysis.py [--sessions 256] [--rounds 3] [--top 3] [--depth 8] [--reps 15] [--out FILE]

Every session is human-first; `rounds` scripted rounds (a seeded random legal human move, the bot's 40 x 8 answer) bring
it to a mid-game position with a searched kept tree, untimed; the sessions then sit on the human's turn.  Timed, each as
one wall-clock interval that begins after a device synchronisation and ends with host-visible results, `reps` times after
two warm-up calls, the median reported:
  device   pool.analyse(sessions, searches=0, top, depth) -- one launch, one host wait;
  host     the walk over engine.lookup in its most favourable form: ONE lookup per depth level for all the lines of all
           the sessions still running (at most depth + 1 launches and host waits), the positions advanced with the
           game's Python rules in between.  (Walking line by line costs a launch and a wait per level per line.)
Both produce the same lines (asserted).  One JSON document on stdout (and in --out)."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
WEIGHTS = os.path.join(ROOT, "caro_ai_amd", "data", "weights", "best_026_12000.dat")


def host_walk(game, eng, sessions, top, depth):
    """[(root_visits or None, [(moves, end)])] per session, by level-synchronous lookups"""
    rows = eng.lookup([s.slot for s in sessions], [0] * len(sessions), [s.state for s in sessions])
    out, lines = [], []  # a running line: [session index, line index, state, mover, node row N, next action]
    for i, s in enumerate(sessions):
        if not rows["found"][i]:
            out.append((None, []))
            continue
        N = rows["N"][i]
        heads = [int(a) for a in np.lexsort((np.arange(len(N)), -N.astype(np.int64))) if N[a] > 0][:top]
        out.append((int(N.sum()), [([], None) for _ in heads]))
        lines += [[i, j, s.state, s.to_move, a] for j, a in enumerate(heads)]
    while lines:
        probe = []
        for ln in lines:
            i, j, state, who, a = ln
            moves = out[i][1][j][0]
            moves.append(a)
            state, won = game.move(state, a, who)
            end = "win" if won else "draw" if not game.possible_moves(state) else "depth" if len(moves) == depth else None
            if end:
                out[i][1][j] = (moves, end)
            else:
                ln[2], ln[3] = state, 1 - who
                probe.append(ln)
        lines = []
        if probe:
            rows = eng.lookup([sessions[ln[0]].slot for ln in probe], [0] * len(probe), [ln[2] for ln in probe])
            for k, ln in enumerate(probe):
                N = rows["N"][k]
                if rows["found"][k] and N.max() > 0:
                    ln[4] = int(np.argmax(N))
                    lines.append(ln)
                else:
                    out[ln[0]][1][ln[1]] = (out[ln[0]][1][ln[1]][0], "leaf")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--top", type=int, default=3)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from caro_ai_amd.lib.game.connect_four import ConnectFour
    from caro_ai_amd.lib.session_pool import SessionPool
    game = ConnectFour()
    M = args.sessions
    pool = SessionPool(game, WEIGHTS, slots=M, device="cuda:0", seed=7)
    eng = pool.engine
    rng = random.Random(1000 + M)
    sessions = [pool.open(True) for _ in range(M)]
    for _ in range(args.rounds):  # (three plies by each side never end a connect four game)
        for s in sessions:
            s.move_player(rng.choice(game.possible_moves(s.state)))
        pool.move_bots(sessions)
    assert all(not s.finished and s.to_move == s.USER_PLAYER for s in sessions)

    def timed(fn):
        for _ in range(2):
            result = fn()
        t = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            result = fn()
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        t = np.array(t) * 1e3
        return result, {"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max())}

    dev, dev_ms = timed(lambda: pool.analyse(sessions, searches=0, top=args.top, depth=args.depth))
    host, host_ms = timed(lambda: host_walk(game, eng, sessions, args.top, args.depth))
    same = all(a.root_visits == h[0] and [(list(ln.moves), ln.end) for ln in a.lines] == h[1] for a, h in zip(dev, host))
    assert same, "the device read-out and the host walk disagree"
    steps = [len(ln.moves) for a in dev for ln in a.lines]
    out = {"what": "SessionPool.analyse(searches=0) against the level-synchronous host walk over SelfPlayEngine.lookup, "
                   "connect four, best_026_12000.dat, sessions on the human's turn after %d scripted rounds of 40 x 8 "
                   "bot moves; median wall ms of one read-out of all sessions" % args.rounds,
           "device": torch.cuda.get_device_name(0), "sessions": M, "top": args.top, "depth": args.depth,
           "reps": args.reps, "lines": len(steps), "mean_line_length": float(np.mean(steps)) if steps else 0.0,
           "analyse_ms": dev_ms, "host_walk_ms": host_ms, "ratio": host_ms["ms_median"] / dev_ms["ms_median"],
           "same_lines": bool(same), "overflows": int(eng.counters()["overflows"]),
           "command": "python tools/measure_analysis.py --sessions %d --rounds %d --top %d --depth %d --reps %d"
                      % (M, args.rounds, args.top, args.depth, args.reps)}
    pool.close_pool()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
