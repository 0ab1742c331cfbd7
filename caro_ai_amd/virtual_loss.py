"""Virtual loss: the rule of include/caro_hip.h, section "virtual loss", in plain numpy -- float64 and float32 exactly
where the kernels use them.  The kernels and the host helper (caro_host_vl_level) share one C++ statement of the
per-action piece; this module is the independent one the tests compare them with, written from the header's text.
"""
import math

import numpy as np

from caro_ai_amd import _lib
from caro_ai_amd import forced_playouts as fp
from caro_ai_amd import fpu as fpu_mod

N_MAX = 16


def check_n(n):
    """n_vl as caro_engine_set_virtual_loss takes it: an integer in [0, 16] (0 = off); anything else raises ValueError"""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= int(n) <= N_MAX:
        raise ValueError("virtual loss must be an integer in [0, %d], got %r" % (N_MAX, n))
    return int(n)


def level_scores(root, N, W, Q, P, strong, legal, noise, c_puct, explore, c, n_vl, q_up=0.0, reduction=0.0):
    """The scores of one level of a descent under the rule, with the counts c[A] of the rule given: float64 at the root
    level (root != 0, `noise` the descent's Dirichlet row), float32 below it.  `reduction` > 0: first-play urgency on top
    (the level's own reduction; `q_up` as caro_ai_amd.fpu takes it).  Illegal actions score -infinity."""
    N = np.asarray(N, np.int64)
    P = np.asarray(P, np.float32)
    legal = np.asarray(legal, bool)
    v = int(n_vl) * np.asarray(c, np.int64)
    N1 = N + v
    nsum1 = int(N1.sum())
    r = np.float64(reduction)
    on = float(reduction) > 0.0
    s = fpu_mod.visited_sqrt(fpu_mod.visited_mass(N, P, legal)) if on else np.float64(0.0)  # (the real row)
    if root:
        qd = fpu_mod.edge_q(N, W, Q, strong)
        q0 = np.where(N > 0, qd, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            qv = ((q0 * N.astype(np.float64)) - v.astype(np.float64)) / N1.astype(np.float64)
        qd = np.where(v > 0, qv, qd)
        if on:
            base = fpu_mod.root_base(N, W, Q, strong)
            qd = np.where(N1 == 0, base - (r * s), qd)
        prob = fp.noised_prior(P, noise, explore)
        sq = np.float64(math.sqrt(nsum1))
        u = ((np.float64(np.float32(c_puct)) * prob) * sq) / (1 + N1).astype(np.float64)
        sc = qd + u
        return np.where(legal, sc, -np.inf)
    q = np.asarray(Q, np.float32).copy()
    q0 = np.where(N > 0, q, np.float32(0.0)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = (q0 * N.astype(np.float32)).astype(np.float32)
        dd = (w - v.astype(np.float32)).astype(np.float32)
        qv = (dd / N1.astype(np.float32)).astype(np.float32)
    q = np.where(v > 0, qv, q).astype(np.float32)
    if on:
        base = np.float32(-np.float32(q_up))
        sub = np.float32(np.float64(base) - (r * s))
        q = np.where(N1 == 0, sub, q).astype(np.float32)
    sqf = np.float32(math.sqrt(nsum1))
    tt = np.float32(c_puct) * P
    tt = tt * sqf
    tt = tt / (1 + N1).astype(np.float32)
    sc = (q + tt).astype(np.float32)
    assert tt.dtype == np.float32
    return np.where(legal, sc, np.float32(-np.inf)).astype(np.float32)


def level_choice(root, N, W, Q, P, strong, legal, noise, c_puct, explore, c, n_vl, q_up=0.0, reduction=0.0, fk=0.0):
    """the action the level takes: the first maximum of level_scores; at the root level with forced playouts (`fk` > 0)
    the lowest forced action, the forced test reading N' and nsum'"""
    if root and fk > 0.0:
        N1 = np.asarray(N, np.int64) + int(n_vl) * np.asarray(c, np.int64)
        f = fp.forced_root(N1, P, noise, legal, explore, fk)
        if f.any():
            return int(np.argmax(f))
    return int(np.argmax(level_scores(root, N, W, Q, P, strong, legal, noise, c_puct, explore, c, n_vl, q_up, reduction)))


def minibatch_choices(B, row_of, legal_of, child_of, root_key, noise, c_puct, explore, n_vl, reduction=0.0,
                      root_reduction=0.0, fk=0.0, max_depth=1 << 30):
    """Replays the B descents of one minibatch in order on frozen rows.  row_of(key) -> dict(N, W, Q, P, strong) or None
    (the board is not in the tree: the descent's leaf); legal_of(key) -> bool[A]; child_of(key, a) -> (key of the board
    after a, ended) with hashable keys; noise[b] the Dirichlet row of descent b.  Returns the B paths as lists of
    (key, action); the counts of descent b are those of the paths 0 .. b-1, an edge once per path."""
    counts = {}
    paths = []
    for b in range(B):
        key, path, q_up = root_key, [], np.float32(0.0)
        while len(path) < max_depth:
            row = row_of(key)
            if row is None:
                break
            root = not path
            A = len(row["N"])
            c = np.array([counts.get((key, a), 0) for a in range(A)], np.int64)
            a = level_choice(root, row["N"], row["W"], row["Q"], row["P"], row["strong"], legal_of(key),
                             noise[b] if root else None, c_puct, explore, c, n_vl, q_up,
                             root_reduction if root else reduction, fk if root else 0.0)
            q_up = fpu_mod.raw_q_up(root, a, row["N"], row["W"], row["Q"], row["strong"])
            path.append((key, a))
            key, ended = child_of(key, a)
            if ended:
                break
        for edge in set(path):
            counts[edge] = counts.get(edge, 0) + 1
        paths.append(path)
    return paths


def host_level(root, N, W, Q, P, strong, legal, noise, c_puct, explore, c, n_vl):
    """caro_host_vl_level: (choice, scores float64[A])"""
    L = _lib.load()
    N = np.ascontiguousarray(N, np.int32)
    W = np.ascontiguousarray(W, np.float32)
    Q = np.ascontiguousarray(Q, np.float32)
    P = np.ascontiguousarray(P, np.float32)
    strong = np.ascontiguousarray(strong, np.int32)
    legal = np.ascontiguousarray(legal, np.uint8)
    c = np.ascontiguousarray(c, np.int32)
    nz = np.ascontiguousarray(noise, np.float64) if noise is not None else None
    out = np.zeros(len(N), np.float64)
    rc = L.caro_host_vl_level(len(N), int(bool(root)), N.ctypes.data, W.ctypes.data, Q.ctypes.data, P.ctypes.data,
                              strong.ctypes.data, legal.ctypes.data, nz.ctypes.data if nz is not None else None,
                              float(c_puct), float(explore), c.ctypes.data, int(n_vl), out.ctypes.data)
    if rc < 0:
        _lib.check(rc)
    return rc, out
