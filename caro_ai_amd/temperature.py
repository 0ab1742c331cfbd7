"""Move temperature and visit-count policy targets: the rule of include/caro_hip.h, section "temperature", in plain numpy
-- float64 with elementwise + - * / and bit views only, in the order the header gives.  The kernels and the host helper
(caro_host_temperature) share one C++ statement of the weight; this module is the independent one the tests compare them
with, written from the header's text.  caro_log and caro_exp are those of include/caro_noise.h, restated.

The rule itself runs in the engine (caro_engine_set_temperature).  Nothing here but host_policy needs the library, and
nothing needs a GPU."""
import numpy as np

from caro_ai_amd import _lib

TAU_MIN, TAU_MAX = 0.05, 8.0
OFF = (1.0, 0.0, False)


def check_tau(tau):
    """a temperature as the engine takes it: 0 or in [0.05, 8] (ValueError otherwise, NaN included)"""
    if isinstance(tau, bool) or not isinstance(tau, (int, float, np.integer, np.floating)):
        raise ValueError("a temperature must be a number, got %r" % (tau,))
    t = float(tau)
    if not (t == 0.0 or TAU_MIN <= t <= TAU_MAX):
        raise ValueError("a temperature must be 0 or in [%g, %g], got %r" % (TAU_MIN, TAU_MAX, tau))
    return t


def check_triple(early=1.0, late=0.0, visit_targets=False):
    """(tau_early, tau_late, visit_targets) as caro_engine_set_temperature takes it; visit_targets is a bool or 0 / 1"""
    if not isinstance(visit_targets, (bool, np.bool_)) and not (isinstance(visit_targets, (int, np.integer))
                                                                 and int(visit_targets) in (0, 1)):
        raise ValueError("visit_targets must be a bool, got %r" % (visit_targets,))
    return check_tau(early), check_tau(late), bool(visit_targets)


def is_on(triple):
    """the feature is ON iff the triple is not (1, 0, False)"""
    return tuple(triple) != OFF


def ply_temperatures(step, sbt0, early=1.0, late=0.0, visit_targets=False):
    """(tau_m, tau_t) of a ply with `step` searched plies behind it: the ply is EARLY iff sbt0 > 0 and step < sbt0"""
    is_early = sbt0 > 0 and step < sbt0
    tau_m = float(early) if is_early else float(late)
    return tau_m, (1.0 if visit_targets else tau_m)


_MANT = np.uint64(0x000fffffffffffff)
_ONE = np.uint64(0x3ff0000000000000)


def caro_log(x):
    """caro_log of include/caro_noise.h on an array of positive normal doubles"""
    x = np.ascontiguousarray(x, np.float64)
    u = x.view(np.uint64)
    e = ((u >> np.uint64(52)) & np.uint64(0x7ff)).astype(np.int64) - 1023
    m = ((u & _MANT) | _ONE).view(np.float64)
    big = m > 1.4142135623730951
    m = np.where(big, m * 0.5, m)
    e = e + big.astype(np.int64)
    t = (m - 1.0) / (m + 1.0)
    t2 = t * t
    s = np.full(x.shape, 1.0 / 25.0)
    for d in (23.0, 21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        s = s * t2 + 1.0 / d
    s = s * t2 + 1.0
    return (2.0 * t) * s + e.astype(np.float64) * 0.6931471805599453


def caro_exp(x):
    """caro_exp of include/caro_noise.h on an array of doubles (0 below -700, clamped at 700)"""
    x = np.ascontiguousarray(x, np.float64)
    zero = x < -700.0
    x = np.where(zero, 0.0, np.where(x > 700.0, 700.0, x))
    kf = x * 1.4426950408889634
    kd = np.trunc(kf + np.where(kf >= 0.0, 0.5, -0.5))  # (long long): towards zero
    k = kd.astype(np.int64)
    r = (x - kd * 6.93147180369123816490e-01) - kd * 1.90821492927058770002e-10
    p = np.full(x.shape, 1.0 / 87178291200.0)
    for c in (6227020800.0, 479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0):
        p = p * r + 1.0 / c
    p = p * r + 0.5
    p = p * r + 1.0
    p = p * r + 1.0
    scale = ((k + 1023).astype(np.uint64) << np.uint64(52)).view(np.float64)
    return np.where(zero, 0.0, p * scale)


def weights(N, tau):
    """w_a of the rule for a tau that is neither 0 nor 1: 0 where N == 0, 1 at the maximum, exp(log(N / nmax) / tau)"""
    N = np.asarray(N, np.int64).ravel()
    nmax = int(N.max())
    w = np.zeros(N.shape, np.float64)
    w[N == nmax] = 1.0
    mid = (N > 0) & (N != nmax)
    if mid.any():
        ratio = N[mid].astype(np.float64) / np.float64(nmax)
        w[mid] = caro_exp(caro_log(ratio) / np.float64(tau))
    return w


def policy(N, tau):
    """T(N, tau): float64[A].  A row without visits has no policy at tau > 0 (ValueError: a refused ply); at tau = 0 it
    is the one-hot at action 0."""
    N = np.asarray(N, np.int64).ravel()
    tau = check_tau(tau)
    tot = int(N.sum())
    if tau == 0.0:
        pi = np.zeros(N.shape, np.float64)
        pi[int(np.argmax(N))] = 1.0  # first maximum
        return pi
    if tot <= 0:
        raise ValueError("a row without visits has no policy at tau > 0")
    if tau == 1.0:
        return N.astype(np.float64) / np.float64(tot)
    w = weights(N, tau)
    S = np.float64(0.0)
    for x in w:  # sequentially, in action order
        S = S + x
    return w / S


def onehot_share(pi):
    """of the rows of pi [n, A]: the share with a single non-zero entry (0.0 for no rows)"""
    pi = np.asarray(pi)
    if pi.size == 0:
        return 0.0
    pi = pi.reshape(-1, pi.shape[-1])
    return float(((pi != 0).sum(axis=1) == 1).mean())


def host_policy(N, tau):
    """caro_host_temperature: (first maximum of N, pi float64[A]); an argument error raises _lib.CaroError"""
    L = _lib.load()
    N = np.ascontiguousarray(N, np.int32).ravel()
    out = np.zeros(len(N), np.float64)
    rc = L.caro_host_temperature(len(N), N.ctypes.data, float(tau), out.ctypes.data)
    if rc < 0:
        _lib.check(rc)
    return rc, out
