"""The reference for early stop (include/caro_hip.h, "early stop"): a self-play game composed ply by ply on the oracle.
An Oracle's search always starts at sim 0 and cannot be snapshotted, so "the tree after m minibatches of ply i" is a
fresh Oracle that replays plies 0 .. i-1 with their known minibatch counts and then searches m minibatches: quadratic
in the game length, fine at test sizes.  The predicate is the product's caro_ai_amd.early_stop.decided, so this reference
and the host-side counters share one Python statement of the rule; tests/test_early_stop_cpu.py checks that statement
independently (constructed rows, and the rule written out with plain oracle calls on a 3 x 3 game).  Used by tests/test_early_stop_cpu.py and tests/test_gpu_early_stop.py."""
import numpy as np

from caro_ai_amd import early_stop
from oracle.oracle import move_uniform, sample_index


def compose_game(make_oracle, seed, uid, first, S, B, sbt0, min_mb=1, cap=None, early=True, resign_t=None,
                 playthrough=False):
    """make_oracle() -> a fresh Oracle of the game.  Ply i has the budget M = S, or min(fast, S) if `cap` = (p_full,
    fast) classes it fast; at a tau = 0 ply (sbt0 == 0 or step >= sbt0) the first m in [min_mb, M - 2] at which the
    root's N after m minibatches is decided (early_stop.decided) makes the ply run m + 1 minibatches, else M.
    resign_t: the mover resigns at a ply whose root Q of the first-max-N edge is below it (not a playthrough game).
    Returns the game (ply 0 first): states, players, pi, z, q, mb, budget, tau0, full, result, steps, and the
    oracle's counters over the whole game."""
    if cap is not None:
        from caro_ai_amd import _lib
        L = _lib.load()
    hist = []  # (state, player, minibatches) of the plies made

    def tree_at(extra, s, player):
        """a fresh oracle that has searched the plies made so far, and `extra` minibatches of the current one"""
        o = make_oracle()
        o.use_synth_net()
        o.set_stream(seed, uid)
        for j, (sj, pj, nj) in enumerate(hist):
            o.search_batch(nj, B, sj, pj, ply=j)
        if extra:
            o.search_batch(extra, B, s, player, ply=len(hist))
        return o

    o0 = make_oracle()
    s, player, step = o0.initial_state, first, 0
    out = {k: [] for k in ("states", "players", "pi", "q", "mb", "budget", "tau0", "full")}
    resigned = False
    while True:
        i = len(hist)
        tau = 1 if (sbt0 > 0 and step < sbt0) else 0
        full = True if cap is None else bool(L.caro_host_cap_uniform(seed, uid, i) < cap[0])
        M = S if full else min(cap[1], S)
        count = M
        if early and tau == 0:
            for m in range(min_mb, M - 1):
                node = tree_at(m, s, player).get_node(s)
                if early_stop.decided(None if node is None else node["N"], m, M, B, min_mb):
                    count = m + 1
                    break
        o = tree_at(count, s, player)
        node = o.get_node(s)
        pi = o.get_policy(s, tau)
        q = float(node["Q"][int(np.argmax(node["N"]))]) if node is not None else 0.0
        for k, val in zip(("states", "players", "pi", "q", "mb", "budget", "tau0", "full"),
                          (s, player, pi, q, count, M, tau == 0, full)):
            out[k].append(val)
        hist.append((s, player, count))
        if resign_t is not None and not playthrough and q < resign_t:
            result, r, resigned = (-1 if player == 0 else 1), -1, True
            break
        a = sample_index(pi, move_uniform(seed, uid, i))
        s, won = o.move(s, a, player)
        if won:
            result, r = (1 if player == 0 else -1), 1
            break
        player = 1 - player
        if not len(o.possible_moves(s)):
            result, r = 0, 0
            break
        step += 1
    n = len(hist)
    out["z"] = [r if (n - 1 - j) % 2 == 0 else -r for j in range(n)]
    out["pi"] = np.array(out["pi"])
    out.update(result=result, steps=step, resigned=resigned, counters=o.counters())
    return out


def tally(games):
    """the conditions a test states about its composed games: games, games with a cut ply, plies, tau = 0 plies, cut
    plies, minibatches saved / budgeted"""
    cut = [sum(m < b for m, b in zip(g["mb"], g["budget"])) for g in games]
    return {"games": len(games), "games_cut": sum(c > 0 for c in cut), "plies": sum(len(g["mb"]) for g in games),
            "tau0": sum(sum(g["tau0"]) for g in games), "cut": sum(cut),
            "saved": sum(b - m for g in games for m, b in zip(g["mb"], g["budget"])),
            "budget": sum(sum(g["budget"]) for g in games)}
