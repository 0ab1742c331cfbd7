#!/usr/bin/env python3
"""One `SessionPool.move_bots` call for M sessions against M separate `Session.move_bot` calls: Connect4, shipped
best_026_12000.dat, the bot's 40 x 8 simulations per move.

    python tools/measure_session_pool.py [--sizes 1,8,64,256] [--reps 7] [--max-sessions 64] [--out FILE]

Every session is human-first; three scripted rounds (a seeded random legal human move, the bot's answer) bring it to a
mid-game position, untimed.  Then `reps` times: every session gets a human move (untimed) and the bot moves of all M
sessions are timed as one wall-clock interval that ends with host-visible results -- one `move_bots(sessions)` for the
pool, M `move_bot()` calls one after the other for the separate sessions (that code is not touched by the pool: it is
the figure of the engine without it).  A session whose game ends is replaced by a new one scripted to mid-game.  The
median over the reps is reported, and the device memory each form holds (torch.cuda.mem_get_info before and after).
Separate sessions are only built up to --max-sessions (each loads the checkpoint, packs a net and allocates an engine);
a larger M is marked "measured": false and carries the largest measured figure scaled by M, which is what M sequential
calls cost.  One JSON document on stdout (and in --out)."""
import argparse
import gc
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
WEIGHTS = os.path.join(ROOT, "caro_ai_amd", "data", "weights", "best_026_12000.dat")
SCRIPTED_ROUNDS = 3


def used_mib(torch):
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return (total - free) / 2.0 ** 20


class Seat:
    """a session of either kind with whose turn it is"""

    def __init__(self, session):
        self.s, self.users_turn, self.over = session, True, False

    def human(self, game, rng):
        won = self.s.move_player(rng.choice(game.possible_moves(self.s.state)))
        self.users_turn = False
        self.over = bool(won) or not game.possible_moves(self.s.state)

    def answered(self, game, won):
        self.users_turn = True
        self.over = bool(won) or not game.possible_moves(self.s.state)


def measure(game, M, reps, rng, new_session, bot_moves, drop):
    """new_session() -> a human-first session; bot_moves(sessions) -> their won flags; drop(session)"""
    def bots(seats):
        for seat, won in zip(seats, bot_moves([x.s for x in seats])):
            seat.answered(game, won)

    def fresh(n):
        seats = [Seat(new_session()) for _ in range(n)]
        for _ in range(SCRIPTED_ROUNDS):  # (three plies by each side never end a connect four game)
            for x in seats:
                x.human(game, rng)
            bots(seats)
        return seats

    def all_on_the_bots_turn(seats):
        while True:
            for x in seats:
                if x.users_turn and not x.over:
                    x.human(game, rng)
            ended = [x for x in seats if x.over]
            if not ended:
                return seats
            for x in ended:
                drop(x.s)
            seats = [x for x in seats if not x.over] + fresh(len(ended))

    seats = fresh(M)
    times = []
    for _ in range(reps + 1):  # (the first rep pays first-use costs and is dropped)
        seats = all_on_the_bots_turn(seats)
        t0 = time.perf_counter()
        bots(seats)
        times.append(time.perf_counter() - t0)
    for x in seats:
        drop(x.s)
    t = np.array(times[1:]) * 1e3
    return {"ms_median": float(np.median(t)), "ms_min": float(t.min()), "ms_max": float(t.max()), "reps": len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,8,64,256")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-sessions", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from caro_ai_amd.lib.game.connect_four import ConnectFour
    from caro_ai_amd.lib.play_session import Session
    from caro_ai_amd.lib.session_pool import SessionPool
    sizes = [int(x) for x in args.sizes.split(",")]
    game = ConnectFour()
    torch.zeros(1, device="cuda:0")
    rows = []

    # ---- the pool: one engine of max(sizes) slots, one net
    m0 = used_mib(torch)
    pool = SessionPool(game, WEIGHTS, slots=max(sizes), device="cuda:0", seed=7)
    pool_mib = used_mib(torch) - m0
    pooled = {}
    for M in sizes:
        rng = random.Random(1000 + M)
        pooled[M] = measure(game, M, args.reps, rng, lambda: pool.open(True),
                            lambda ss: [r[2] for r in pool.move_bots(ss)], pool.close)
    overflows = pool.engine.counters()["overflows"]
    pool.close_pool()
    del pool
    gc.collect()

    # ---- M separate Sessions, one after the other
    separate, sep_mib = {}, {}
    for M in sizes:
        if M > args.max_sessions:
            continue
        rng = random.Random(1000 + M)
        np.random.seed(1000 + M)
        m0 = used_mib(torch)
        live = []

        def new_session():
            s = Session(game, WEIGHTS, True, device="cuda:0")
            live.append(s)
            return s

        def drop(s):
            live.remove(s)
            if s.mcts_store._eng is not None:
                s.mcts_store._eng.close()
            for _, hip in s.mcts_store._hip.values():
                hip.close()

        peak = [0.0]

        def bot_moves(ss):
            won = [s.move_bot() for s in ss]
            peak[0] = max(peak[0], used_mib(torch) - m0) if len(ss) == M else peak[0]
            return won

        separate[M] = measure(game, M, args.reps, rng, new_session, bot_moves, drop)
        sep_mib[M] = peak[0]
        gc.collect()
        torch.cuda.empty_cache()

    top = max(separate) if separate else None
    for M in sizes:
        row = {"sessions": M, "pool_ms": pooled[M]["ms_median"], "pool_ms_min_max": [pooled[M]["ms_min"], pooled[M]["ms_max"]]}
        if M in separate:
            row.update(separate_ms=separate[M]["ms_median"], separate_ms_min_max=[separate[M]["ms_min"], separate[M]["ms_max"]],
                       separate_mib=sep_mib[M], separate_measured=True)
        elif top is not None:
            row.update(separate_ms=separate[top]["ms_median"] * M / top, separate_mib=sep_mib[top] * M / top,
                       separate_measured=False)
        if "separate_ms" in row:
            row["ratio"] = row["separate_ms"] / row["pool_ms"]
        rows.append(row)
    out = {"what": "SessionPool.move_bots(M sessions) against M Session.move_bot calls, connect four, best_026_12000.dat, "
                   "40 x 8 simulations per move, mid-game positions, median wall ms of one round of M bot moves",
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "pool_slots": max(sizes),
           "pool_device_mib": pool_mib, "pool_overflows": int(overflows), "rows": rows,
           "command": "python tools/measure_session_pool.py --sizes %s --reps %d --max-sessions %d"
                      % (args.sizes, args.reps, args.max_sessions)}  # (what shapes the figures; not where they went)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
