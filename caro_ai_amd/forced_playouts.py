"""Forced playouts and policy target pruning (KataGo, Wu 2019): the two rules of include/caro_hip.h, section "forced
playouts", in plain numpy -- float64 and float32 exactly where the kernels use them -- and the reader of the engine's
four tallies.  The kernels and the host helpers (caro_host_forced_root / caro_host_forced_prune) share one C++ statement
of the rules; this module is the independent one the tests compare them with.
"""
import ctypes as C
import math

import numpy as np

from caro_ai_amd import _lib

K_MAX = 64.0
KATAGO_K = 2.0
STAT_NAMES = ("root_descents", "forced_descents", "pruned_plies", "visits_removed")


def check_k(k):
    """k as caro_engine_set_forced_playouts takes it: a float in [0, 64] (0 = off); anything else raises ValueError"""
    try:
        kf = float(k)
    except (TypeError, ValueError):
        raise ValueError("forced playouts k must be a number in [0, %g], got %r" % (K_MAX, k))
    if isinstance(k, bool) or not 0.0 <= kf <= K_MAX:  # (NaN fails both comparisons)
        raise ValueError("forced playouts k must be in [0, %g], got %r" % (K_MAX, k))
    return kf


def noised_prior(P, noise, explore):
    """prob_a of the root score: float32(1 - explore) * P in float32, widened, + explore * noise in float64"""
    keep = np.float32(1.0 - float(explore)) * np.asarray(P, np.float32)
    assert keep.dtype == np.float32
    return keep.astype(np.float64) + np.float64(explore) * np.asarray(noise, np.float64)


def forced_root(N, P, noise, legal, explore, k):
    """bool[A]: the actions forced at a root with visit counts N, raw priors P and the descent's Dirichlet row"""
    N = np.asarray(N, np.int64)
    n = N.astype(np.float64)
    T = np.float64(int(N.sum()))
    prob = noised_prior(P, noise, explore)
    return np.asarray(legal, bool) & (N > 0) & (n * n < (np.float64(k) * prob) * T)


def root_choice(N, P, noise, legal, explore, k, off_action):
    """the action the root level takes: the lowest forced action, or `off_action` (the usual choice) when none is"""
    f = forced_root(N, P, noise, legal, explore, k)
    return int(np.argmax(f)) if f.any() else int(off_action)


def edge_q(N, W, Q, strong):
    """Q of every edge as the root level of a descent reads it: float32 Q where W is strong, else W / N (0 unvisited)"""
    N = np.asarray(N, np.int64)
    W = np.asarray(W, np.float32).astype(np.float64)
    q = np.where(N > 0, W / np.maximum(N, 1).astype(np.float64), 0.0)
    return np.where(np.asarray(strong) != 0, np.asarray(Q, np.float32).astype(np.float64), q)


def prune(N, Q, P, c_puct, k):
    """(N', b): the pruned visit counts of a root row (Q float64 as edge_q gives it, P raw float32 priors) and the
    first maximum b of N.  The predicate is evaluated count by count, as the rule states it."""
    N = np.asarray(N, np.int64)
    Q = np.asarray(Q, np.float64)
    Pd = np.asarray(P, np.float32).astype(np.float64)
    T = int(N.sum())
    if T <= 0:
        raise ValueError("a row without visits has no policy")
    b = int(np.argmax(N))
    sq = np.float64(math.sqrt(T))
    c = np.float64(np.float32(c_puct))
    k = np.float64(k)

    def score(a, n):
        return Q[a] + ((c * Pd[a]) * sq) / np.float64(1 + n)

    s_star = score(b, int(N[b]))
    out = N.copy()
    for a in range(len(N)):
        na = int(N[a])
        if a == b or na == 0:
            continue
        F = int(math.sqrt((k * Pd[a]) * np.float64(T)))
        new = na
        for n in range(max(0, na - F), na + 1):
            if score(a, n) < s_star:
                new = n
                break
        out[a] = 0 if new == 1 else new
    return out.astype(np.int32), b


def pruned_pi(N, Q, P, c_puct, k):
    """the tuple's pi of a pruned ply: float64 N' / sum N'"""
    n2, _ = prune(N, Q, P, c_puct, k)
    return n2.astype(np.float64) / np.float64(int(n2.sum()))


def host_forced_root(N, P, noise, legal, explore, k):
    """caro_host_forced_root: (forced bool[A], count)"""
    L = _lib.load()
    N = np.ascontiguousarray(N, np.int32)
    P = np.ascontiguousarray(P, np.float32)
    noise = np.ascontiguousarray(noise, np.float64)
    legal = np.ascontiguousarray(legal, np.uint8)
    out = np.zeros(len(N), np.uint8)
    rc = L.caro_host_forced_root(len(N), N.ctypes.data, P.ctypes.data, noise.ctypes.data, legal.ctypes.data,
                                 float(explore), float(k), out.ctypes.data)
    if rc < 0:
        _lib.check(rc)
    return out.astype(bool), rc


def host_forced_prune(N, Q, P, c_puct, k):
    """caro_host_forced_prune: (N' int32[A], b)"""
    L = _lib.load()
    N = np.ascontiguousarray(N, np.int32)
    Q = np.ascontiguousarray(Q, np.float64)
    P = np.ascontiguousarray(P, np.float32)
    out = np.zeros(len(N), np.int32)
    rc = L.caro_host_forced_prune(len(N), N.ctypes.data, Q.ctypes.data, P.ctypes.data, float(c_puct), float(k),
                                  out.ctypes.data)
    if rc < 0:
        _lib.check(rc)
    return out, rc


def stats(engine):
    """caro_forced_stats of a SelfPlayEngine (or the sum over the parts of a StreamedSelfPlay): the four tallies by
    name, plus forced_share = forced / root descents (0 when there were none)"""
    parts = getattr(engine, "parts", None) or [engine]
    tot = [0, 0, 0, 0]
    for e in parts:
        out = (C.c_int64 * 4)()
        _lib.check(e.L.caro_forced_stats(e.h, out, e._stream()))
        tot = [a + int(b) for a, b in zip(tot, out)]
    d = dict(zip(STAT_NAMES, tot))
    d["forced_share"] = d["forced_descents"] / d["root_descents"] if d["root_descents"] else 0.0
    return d


def shares(st, sims):
    """forced_share and pruned_visits_share of a run: forced root descents per root descent under the rule, and visits
    removed from the tuples' pi per simulation the run made (`sims`: counters()["sims"])"""
    return {"forced_share": st["forced_share"],
            "pruned_visits_share": st["visits_removed"] / sims if sims else 0.0}


def entropy(pi):
    """Shannon entropy (nats) of each row of pi, 0 log 0 = 0"""
    pi = np.asarray(pi, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(pi > 0, pi * np.log(pi), 0.0)
    return -t.sum(-1)
