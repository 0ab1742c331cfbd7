#!/usr/bin/env python3
"""What playout cap randomization buys in Connect4 self-play: config 2's shape (1 024 games, 25 x 8 sims per move, the
staggered stream form -- every slot restarts in place -- with the shipped best_026_12000.dat on the fused HIP net)
played with the cap off, at p_full = 1 (flags recorded, nothing else changes) and at (p_full, fast) = (0.25, 5) and
(0.25, 8).  Every setting restarts the engine, plays --warmup passes (one pass = `searches` launches) and then times
--steps passes.  Per setting: plies/s, finished games/s, full tuples/s (tuples of full plies in the finished games),
the full-ply share, and -- from --sample single launches after the window, each followed by caro_pending_leaves -- the
mean and maximum net rows per launch and the share of launches past one round of tiles (256 CUs x 6 boards = 1 536).

    python tools/measure_playout_cap.py [--warmup 40] [--steps 80] [--sample 200]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

ROUND_ROWS = 256 * 6  # one round of the net kernel's tiles


def window(eng, S, B, warmup, steps):
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
    return {k: c1[k] - c0[k] for k in c1}, drains, dt


def launch_rows(eng, B, n):
    """net rows of n single staggered launches (caro_pending_leaves after each: the leaves that launch's net call took)"""
    from caro_ai_amd import _lib
    L = _lib.load()
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rows = []
    for _ in range(n):
        _lib.check(L.caro_search_staggered(eng.h, eng.evaluators[0].h, None, 1, B, ptr(eng.planes), ptr(eng.leaf_keys),
                                           ptr(eng._probs), ptr(eng._values), eng._stream()))
        rows.append(eng.pending_leaves())
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=40, help="passes before the timed window of each setting")
    ap.add_argument("--steps", type=int, default=80, help="passes in the timed window")
    ap.add_argument("--sample", type=int, default=200, help="single launches sampled for the net rows per launch")
    ap.add_argument("--weights", default=os.path.join(ROOT, "tests", "golden", "weights", "best_026_12000.dat"))
    args = ap.parse_args(argv)
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
    eng = None
    for setting in (None, (1.0, 5), (0.25, 5), (0.25, 8)):
        if eng is None or setting is None:  # (the cap cannot be switched off again: the off run gets its own engine)
            if eng is not None:
                eng.close()
            eng = SelfPlayEngine(game, args.games, evaluators=[hip], max_batch=B, steps_before_tau_0=10, seed=seed,
                                 device=device, searches_hint=S, stagger=True)
        else:
            eng.restart(seed=seed)
        if setting is not None:
            eng.set_playout_cap(*setting)
        c, drains, dt = window(eng, S, B, args.warmup, args.steps)
        n_tuples = sum(int(d["z"].shape[0]) for d in drains)
        n_full = sum(int(d["full"].sum()) for d in drains) if setting is not None else n_tuples
        sample = launch_rows(eng, B, args.sample)
        row = {"p_full": None if setting is None else setting[0], "fast": None if setting is None else setting[1],
               "plies_per_s": c["plies"] / dt, "games_per_s": c["finished"] / dt, "full_tuples_per_s": n_full / dt,
               "full_share": n_full / max(n_tuples, 1), "sims_per_ply": c["sims"] / max(c["plies"], 1),
               "net_rows_per_launch": sum(sample) / len(sample), "net_rows_max": max(sample),
               "launches_past_one_round": sum(r > ROUND_ROWS for r in sample) / len(sample), "seconds": dt}
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
    eng.close()
    base = rows[0]
    out = {"config": "connect four, %d games, %dx%d sims/move, staggered stream, %s, hip f32w net"
                     % (args.games, S, B, os.path.basename(args.weights)),
           "warmup_passes": args.warmup, "steps": args.steps, "sampled_launches": args.sample, "runs": rows,
           "vs_off": [{k: r[k] / base[k] for k in ("plies_per_s", "games_per_s", "full_tuples_per_s")} for r in rows]}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
