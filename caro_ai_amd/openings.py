"""Random openings on the host: the rule in plain Python over the game classes (what the engine computes where a game
starts; include/caro_hip.h, "openings"), the argument check of SelfPlayEngine.set_openings, and the counters self-play
reports.

The rule itself runs in the engine (caro_engine_set_openings).  Nothing here needs a GPU."""
import numpy as np

MAX_PLIES = 64
_M64 = (1 << 64) - 1
_TAG = 0x6f70656e  # "open"


def _mix64(z):
    """splitmix64 finaliser (caro_mix64 of include/caro_noise.h)"""
    z ^= z >> 30
    z = (z * 0xbf58476d1ce4e5b9) & _M64
    z ^= z >> 27
    z = (z * 0x94d049bb133111eb) & _M64
    return z ^ (z >> 31)


def open_uniform(seed, uid, i):
    """caro_open_uniform(seed, uid, i) of include/caro_noise.h: i = 0 draws the opening's length, 1 + j its ply j"""
    k = _mix64((int(seed) & _M64) ^ _TAG)
    k = _mix64((k + int(uid)) & _M64)
    k = _mix64(k ^ (int(i) & 0xffffffff))
    return ((k >> 12) + 0.5) * (1.0 / 4503599627370496.0)


def limit(max_plies, cells=None):
    """max_plies as the engine takes it: an integer in [0, 64], below the board's cell count (ValueError otherwise)"""
    m = max_plies
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 0 <= int(m) <= MAX_PLIES:
        raise ValueError("opening plies must be an integer in [0, %d], got %r" % (MAX_PLIES, max_plies))
    if cells is not None and int(m) >= cells:
        raise ValueError("opening plies must be below the board's cell count (%d), got %r" % (cells, max_plies))
    return int(m)


def pair_key(uid):
    """The key of game `uid`'s opening under paired openings (caro_engine_set_opening_pairs): games 2j and 2j + 1 share it"""
    return int(uid) >> 1


def opening(game, seed, uid, first, max_plies, paired=False):
    """The root of game `uid` whose first player is `first`: (state, player to move there, opening plies made).
    r = min(max_plies, floor(u_0 * (max_plies + 1))) plies are tried; ply i plays the legal action of index
    min(L - 1, floor(u_{1+i} * L)) for the side to move, unless that move wins or fills the board: then the opening
    ends and the move is not made.  paired: every u is drawn at pair_key(uid) instead of uid, and nothing else
    changes -- with first = uid & 1 the roots of games 2j and 2j + 1 are colour-swapped twins."""
    if paired:
        uid = pair_key(uid)
    state, player, made = game.initial_state, int(first), 0
    r = min(max_plies, int(open_uniform(seed, uid, 0) * (max_plies + 1)))
    for i in range(r):
        legal = list(game.possible_moves(state))
        j = min(len(legal) - 1, int(open_uniform(seed, uid, 1 + i) * len(legal)))
        nxt, won = game.move(state, legal[j], player)
        if won or not len(game.possible_moves(nxt)):
            break
        state, player, made = nxt, 1 - player, made + 1
    return state, player, made


def open_stats(drains):
    """What self-play reports over a list of drains (host arrays with "games" and "open"): open_games, the games that
    made at least one opening ply, and open_plies_mean, the opening plies per drained game."""
    games = plies = opened = 0
    for d in drains:
        counts = np.asarray(d["games"]).reshape(-1, 4)[:, 3].astype(np.int64) + 1
        op = np.asarray(d["open"]).astype(np.int64)
        assert int(counts.sum()) == len(op), (int(counts.sum()), len(op))
        per_game = op[np.cumsum(counts) - counts] if len(counts) else op[:0]  # constant within a game: its first row
        games += len(counts)
        plies += int(per_game.sum())
        opened += int((per_game > 0).sum())
    return {"open_games": opened, "open_plies_mean": plies / games if games else 0.0}
