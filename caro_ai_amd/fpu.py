"""First-play urgency reduction: the rule of include/caro_hip.h, section "first-play urgency", in plain numpy -- float64
and float32 exactly where the kernels use them.  The kernels and the host helper (caro_host_fpu_level) share one C++
statement of the per-action pieces; this module is the independent one the tests compare them with, written from the
header's text.
"""
import math

import numpy as np

from caro_ai_amd import _lib

R_MAX = 2.0
MASS_ONE = 4194304.0  # 2^22


def check_reduction(r, name="reduction"):
    """a reduction as caro_engine_set_fpu takes it: a float in [0, 2] (0 = off); anything else raises ValueError"""
    try:
        rf = float(r)
    except (TypeError, ValueError):
        raise ValueError("fpu %s must be a number in [0, %g], got %r" % (name, R_MAX, r))
    if isinstance(r, bool) or not 0.0 <= rf <= R_MAX:  # (NaN fails both comparisons)
        raise ValueError("fpu %s must be in [0, %g], got %r" % (name, R_MAX, r))
    return rf


def check_pair(fpu):
    """the `fpu=` keyword of train: None, a number r (both reductions) or (r, r_root) -> (r, r_root) floats"""
    if isinstance(fpu, (tuple, list)):
        if len(fpu) != 2:
            raise ValueError("fpu must be a reduction or (reduction, root_reduction), got %r" % (fpu,))
        r, rr = fpu
    else:
        r, rr = fpu, None
    r = check_reduction(r)
    return r, (r if rr is None else check_reduction(rr, "root reduction"))


def visited_mass(N, P, legal):
    """M: the int32 sum over legal visited actions of m_a = floor(clamp(P[a], 0, 1) * 2^22)"""
    P = np.asarray(P, np.float32)
    with np.errstate(invalid="ignore"):
        c = np.minimum(np.maximum(P, np.float32(0.0)), np.float32(1.0))
    c = np.where(np.isnan(P), np.float32(0.0), c).astype(np.float32)
    m = np.floor(c * np.float32(MASS_ONE)).astype(np.int64)
    sel = np.asarray(legal, bool) & (np.asarray(N, np.int64) > 0)
    return int(m[sel].sum())


def visited_sqrt(M):
    """s = SQRT((double)M * 2^-22)"""
    return np.float64(math.sqrt(float(M) * (1.0 / MASS_ONE)))


def edge_q(N, W, Q, strong):
    """Q of every edge as the root level reads it (float64): the float32 Q word where the strong flag is set, else
    W / N in float64, 0 without visits"""
    N = np.asarray(N, np.int64)
    W = np.asarray(W, np.float32).astype(np.float64)
    q = np.where(N > 0, W / np.maximum(N, 1).astype(np.float64), 0.0)
    return np.where(np.asarray(strong) != 0, np.asarray(Q, np.float32).astype(np.float64), q)


def root_base(N, W, Q, strong):
    """the root Q of the row (section "resignation"): the first maximum of N and that edge's Q, 0 without visits"""
    N = np.asarray(N, np.int64)
    b = int(np.argmax(N))
    return np.float64(edge_q(N, W, Q, strong)[b]) if N[b] > 0 else np.float64(0.0)


def raw_q_up(root, a, N, W, Q, strong):
    """q_up for the level below: the raw Q of edge `a` as this level read it, rounded to float32"""
    if root:
        return np.float32(edge_q(N, W, Q, strong)[a])
    return np.float32(np.asarray(Q, np.float32)[a])


def level_scores(root, N, W, Q, P, strong, legal, noise, c_puct, explore, q_up, reduction):
    """The scores of one level of a descent under the rule: float64 at the root level (root != 0, `noise` the descent's
    Dirichlet row), float32 below it (`q_up` the raw Q of the edge taken one level up; `noise` unused).  `reduction` is
    the level's own (r_root at the root, r below); 0 gives today's scores.  Illegal actions score -infinity."""
    N = np.asarray(N, np.int64)
    P = np.asarray(P, np.float32)
    legal = np.asarray(legal, bool)
    nsum = int(N.sum())
    r = np.float64(reduction)
    on = float(reduction) > 0.0
    s = visited_sqrt(visited_mass(N, P, legal)) if on else np.float64(0.0)
    if root:
        qd = edge_q(N, W, Q, strong)
        if on:
            base = root_base(N, W, Q, strong)
            qd = np.where(N == 0, base - (r * s), qd)
        keep = np.float32(1.0 - float(explore)) * P
        prob = keep.astype(np.float64) + np.float64(explore) * np.asarray(noise, np.float64)
        sq = np.float64(math.sqrt(nsum))
        u = ((np.float64(np.float32(c_puct)) * prob) * sq) / (1 + N).astype(np.float64)
        sc = qd + u
        return np.where(legal, sc, -np.inf)
    q = np.asarray(Q, np.float32).copy()
    if on:
        base = np.float32(-np.float32(q_up))
        sub = np.float32(np.float64(base) - (r * s))
        q = np.where(N == 0, sub, q).astype(np.float32)
    sqf = np.float32(math.sqrt(nsum))
    tt = np.float32(c_puct) * P
    tt = tt * sqf
    tt = tt / (1 + N).astype(np.float32)
    sc = (q + tt).astype(np.float32)
    assert tt.dtype == np.float32
    return np.where(legal, sc, np.float32(-np.inf)).astype(np.float32)


def level_choice(root, N, W, Q, P, strong, legal, noise, c_puct, explore, q_up, reduction):
    """the action the level takes: the first maximum of level_scores"""
    return int(np.argmax(level_scores(root, N, W, Q, P, strong, legal, noise, c_puct, explore, q_up, reduction)))


def host_level(root, N, W, Q, P, strong, legal, noise, c_puct, explore, q_up, reduction):
    """caro_host_fpu_level: (choice, scores float64[A])"""
    L = _lib.load()
    N = np.ascontiguousarray(N, np.int32)
    W = np.ascontiguousarray(W, np.float32)
    Q = np.ascontiguousarray(Q, np.float32)
    P = np.ascontiguousarray(P, np.float32)
    strong = np.ascontiguousarray(strong, np.int32)
    legal = np.ascontiguousarray(legal, np.uint8)
    nz = np.ascontiguousarray(noise, np.float64) if noise is not None else None
    out = np.zeros(len(N), np.float64)
    rc = L.caro_host_fpu_level(len(N), int(bool(root)), N.ctypes.data, W.ctypes.data, Q.ctypes.data, P.ctypes.data,
                               strong.ctypes.data, legal.ctypes.data, nz.ctypes.data if nz is not None else None,
                               float(c_puct), float(explore), float(q_up), float(reduction), out.ctypes.data)
    if rc < 0:
        _lib.check(rc)
    return rc, out
