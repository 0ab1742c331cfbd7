"""The reference for arena games from random openings (include/caro_hip.h, "openings", caro_engine_set_opening_pairs): a
game between two table nets composed ply by ply on the oracle from its opened root.  It follows
tests/openings_ref.compose_game_from, for the arena: one oracle with two stores and the two salted table nets; player
p's tree (store p) is searched only at p's own plies, its leaves go to net p (oracle_play_game's arena rule); the root
is the product's plain-Python statement of the rule, caro_ai_amd.openings.opening(..., paired=...).  The searched plies
number from 0 at the opened root: the noise keys are (seed, uid, ply, sim) and the move uniform is ply's, all on the
game's own uid -- only the opening is keyed by the pair.  Used by tests/test_gpu_arena_openings.py."""
import numpy as np

from caro_ai_amd import openings
from oracle.oracle import move_uniform, sample_index


def compose_arena_game(make_oracle, game, seed, uid, first, max_plies, S, B, sbt0, salts, paired=True):
    """make_oracle() -> a fresh Oracle of `game` with two stores.  Returns the game (tuple 0 first): states, players,
    pi, z, open, first (the mover of tuple 0), result (+1: player 0, net salts[0], won), steps and the oracle's counters."""
    o = make_oracle()
    o.use_synth_net(*salts)
    o.set_stream(seed, uid)
    s, player, made = openings.opening(game, seed, uid, first, max_plies, paired=paired)
    out = {"states": [], "players": [], "pi": [], "open": made, "first": player}
    step = 0
    while True:
        i = len(out["states"])
        tau = 1 if (sbt0 > 0 and step < sbt0) else 0
        o.search_batch(S, B, s, player, store=player, which_net=player, ply=i)
        pi = o.get_policy(s, tau, store=player)
        out["states"].append(s)
        out["players"].append(player)
        out["pi"].append(pi)
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
    n = len(out["states"])
    out["z"] = [r if (n - 1 - j) % 2 == 0 else -r for j in range(n)]
    out["pi"] = np.array(out["pi"])
    out.update(result=result, steps=step, counters=o.counters())
    return out
