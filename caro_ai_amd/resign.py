"""Resignation bookkeeping on the host: per-game sequences from a drain, the false-positive rate of a threshold, and its
calibration (AlphaGo Zero's v_resign: a share of games plays through regardless, and those games measure how often a
resignation would have been wrong).

The rule itself runs in the engine's ply (include/caro_hip.h, "resignation"; SelfPlayEngine.set_resign).  A game here
is a dict with, in GAME order (ply 0 first): "q" the root Q of every ply (mover's view), "z" the outcome from that ply's
mover's view (+1 won, 0 draw, -1 lost), "players" (and "states", "pi", "full", "mb", "open" when the drain has them); and "uid", "first",
"result", "steps" (the drain's game record), "resigned" (the game ended by resignation) and "playthrough" (the game
could not resign; None if unknown).
"""
import numpy as np

from caro_ai_amd import _lib


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def split_games(drain, seed=None, playthrough=None):
    """A drain's flat rows (each game's plies last to first, games in record order) -> a list of per-game dicts in
    game order.  A game has steps + 1 tuples: every ply but the last (a win, a draw or a resignation) advances the
    record's steps.  With `seed` and `playthrough` (the engine's) each game is marked as a playthrough game or not."""
    recs = _host(drain["games"]).reshape(-1, 4)
    z = _host(drain["z"])
    players = _host(drain["players"])
    q = _host(drain["root_q"]) if "root_q" in drain else None
    counts = recs[:, 3].astype(np.int64) + 1
    if int(counts.sum()) != len(z):
        raise ValueError("split_games: %d rows, but the game records account for %d" % (len(z), int(counts.sum())))
    L = _lib.load() if seed is not None else None
    games, off = [], 0
    for (uid, first, result, steps), n in zip(recs.tolist(), counts.tolist()):
        rows = slice(off, off + n)
        off += n
        zg = z[rows][::-1].astype(np.int64)
        g = {"uid": int(uid), "first": int(first), "result": int(result), "steps": int(steps),
             "z": zg, "players": players[rows][::-1].astype(np.int64),
             "q": q[rows][::-1].astype(np.float64) if q is not None else None,
             "resigned": bool(zg[-1] == -1),  # the last mover lost: it resigned (a winning ply has z = +1)
             "playthrough": None}
        # (when the drain has them; "full": the playout cap's ply classes, "mb": early stop's minibatches per ply, "open":
        # the opening plies the game made, the same in every row)
        for k in ("states", "pi", "full", "mb", "open"):
            if k in drain:
                g[k] = _host(drain[k])[rows][::-1]
        if L is not None:
            g["playthrough"] = bool(L.caro_host_resign_uniform(int(seed) & (2 ** 64 - 1), int(uid)) < playthrough)
        games.append(g)
    return games


def _trigger(g, t):
    """index of the first ply (game order) with q < t, or None"""
    hit = np.flatnonzero(np.asarray(g["q"]) < t)
    return int(hit[0]) if len(hit) else None


def false_positive_rate(games, t):
    """FP(t) over the playthrough games: of those in which some ply has q < t, the share in which the mover of the FIRST
    such ply did not lose (a draw counts as a false positive).  0 if no playthrough game has such a ply."""
    trig = fp = 0
    for g in games:
        if not g["playthrough"]:
            continue
        i = _trigger(g, t)
        if i is None:
            continue
        trig += 1
        fp += int(g["z"][i] != -1)
    return fp / trig if trig else 0.0


def calibrate(games, target_fp, current, min_games=20):
    """The largest candidate threshold t with FP(t) <= target_fp.  Candidates: -1 (which never triggers) and
    nextafter(q, +inf) of every root Q recorded in a playthrough game (the smallest t at which that ply triggers), those
    above 1 left out (the engine's thresholds lie in [-1, 1]).  Fewer than `min_games` playthrough games: `current`."""
    pt = [g for g in games if g["playthrough"]]
    if len(pt) < min_games:
        return current
    qs = np.concatenate([np.asarray(g["q"], np.float64) for g in pt]) if pt else np.zeros(0)
    cand = np.nextafter(qs, np.inf)
    cand = np.unique(np.concatenate([[-1.0], cand[cand <= 1.0]]))
    # Sweep: in a game the trigger at t is the first ply whose q is below t, i.e. the first new prefix minimum below t.
    # With the prefix minima r_0 > r_1 > ... (first seen at plies i_0 < i_1 < ...), t in (r_j, r_{j-1}] triggers at
    # ply i_j (r_{-1} = +inf); every such interval adds one trigger, and one false positive if its mover did not lose.
    ntrig = np.zeros(len(cand) + 1, np.int64)
    nfp = np.zeros(len(cand) + 1, np.int64)
    for g in pt:
        q = np.asarray(g["q"], np.float64)
        z = np.asarray(g["z"])
        hi = np.inf
        m = np.inf
        for i in range(len(q)):
            if q[i] < m:
                m = q[i]
                lo_i = np.searchsorted(cand, m, side="right")   # first candidate > m
                hi_i = np.searchsorted(cand, hi, side="right")  # first candidate > hi
                ntrig[lo_i] += 1
                ntrig[hi_i] -= 1
                if z[i] != -1:
                    nfp[lo_i] += 1
                    nfp[hi_i] -= 1
                hi = m
    ntrig = np.cumsum(ntrig)[:-1]
    nfp = np.cumsum(nfp)[:-1]
    fp = np.where(ntrig > 0, nfp / np.maximum(ntrig, 1), 0.0)
    ok = np.flatnonzero(fp <= target_fp)
    return float(cand[ok[-1]])


def summary(games, t):
    """what train.fit logs: the share of all games that resigned, and FP(t) over the playthrough games"""
    n = len(games)
    return {"resign_fraction": sum(g["resigned"] for g in games) / n if n else 0.0,
            "resign_false_positive": false_positive_rate(games, t)}
