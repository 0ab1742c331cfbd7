"""Move temperature and visit-count policy targets on the host (include/caro_hip.h, "temperature"): the C helper
caro_host_temperature -- the statement of T(N, tau) the kernels share -- against the independent numpy statement
(caro_ai_amd/temperature.py), bit for bit; the rule's meaning against the reference's `count ** (1 / tau)` normalised;
argument errors; the two temperatures of a ply.  No GPU."""
import numpy as np
import pytest

from caro_ai_amd import _lib
from caro_ai_amd import temperature as tp

ACTIONS = (7, 9, 81, 225)
TAUS = (0.0, 0.05, 0.25, 0.5, 1.0, 1.25, 2.0, 8.0)


def _rows(A, rng, hi=1 << 20):
    """count rows over A actions: random ones, ones full of zeros, ties at the maximum, a single visited action"""
    rows = [rng.integers(0, hi + 1, A) for _ in range(6)]
    rows += [rng.integers(0, 40, A) for _ in range(6)]  # (small counts: the rows a short search leaves)
    sparse = rng.integers(0, hi + 1, A)
    sparse[rng.random(A) < 0.6] = 0
    sparse[int(rng.integers(A))] = hi
    rows.append(sparse)
    tie = rng.integers(0, 1000, A)
    tie[[1, A // 2, A - 1]] = 1000  # three maxima: the first one counts
    rows.append(tie)
    one = np.zeros(A, np.int64)
    one[int(rng.integers(A))] = int(rng.integers(1, hi))
    rows.append(one)
    last = np.zeros(A, np.int64)
    last[A - 1] = 1
    rows.append(last)
    rows.append(np.full(A, 3))  # all equal
    return [np.asarray(r, np.int64) for r in rows]


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


@pytest.mark.parametrize("A", ACTIONS)
def test_host_helper_equals_the_numpy_rule_bit_for_bit(A):
    rng = np.random.default_rng(100 + A)
    for N in _rows(A, rng):
        for tau in TAUS:
            best, pi = tp.host_policy(N, tau)
            want = tp.policy(N, tau)
            assert best == int(np.argmax(N))
            assert np.array_equal(_bits(pi), _bits(want)), (A, tau, N.tolist())
            assert (pi[N == 0] == 0).all() and (tau == 0.0 or (pi[N > 0] > 0).all())
            assert abs(pi.sum() - 1.0) < 1e-12


@pytest.mark.parametrize("A", ACTIONS)
def test_tau_one_is_the_visit_share_and_tau_zero_the_first_maximum(A):
    rng = np.random.default_rng(200 + A)
    for N in _rows(A, rng):
        _, pi1 = tp.host_policy(N, 1.0)
        assert np.array_equal(_bits(pi1), _bits(N.astype(np.float64) / np.float64(int(N.sum()))))
        assert np.array_equal(_bits(tp.policy(N, 1.0)), _bits(pi1))
        b, pi0 = tp.host_policy(N, 0.0)
        onehot = np.zeros(A)
        onehot[int(np.argmax(N))] = 1.0  # numpy's argmax is the first maximum
        assert b == int(np.argmax(N)) and np.array_equal(_bits(pi0), _bits(onehot))
        assert np.array_equal(_bits(tp.policy(N, 0.0)), _bits(onehot))


@pytest.mark.parametrize("A", ACTIONS)
def test_the_rule_is_the_references_formula(A):
    """a guard on the rule's meaning: count ** (1 / tau) normalised with Python floats (lib/mcts.py:305-311), counts up
    to 12 800 and tau >= 0.25 so that the power does not overflow; every non-zero entry within 1e-12 relative"""
    rng = np.random.default_rng(300 + A)
    worst = 0.0
    for N in _rows(A, rng, hi=12800):
        for tau in (0.25, 0.5, 1.0, 1.25, 2.0, 8.0):
            counts = [float(int(c)) ** (1.0 / tau) for c in N]
            total = sum(counts)
            ref = np.array([c / total for c in counts])
            _, pi = tp.host_policy(N, tau)
            nz = ref != 0
            assert ((pi != 0) == nz).all()
            rel = np.abs(pi[nz] - ref[nz]) / ref[nz]
            worst = max(worst, float(rel.max()))
            assert rel.max() <= 1e-12, (A, tau, float(rel.max()))
    print("temperature against count ** (1 / tau), A = %d: worst relative difference %.3g" % (A, worst))


def test_the_weights_are_the_power():
    """caro_log / caro_exp as restated in numpy: a weight is (n / nmax) ** (1 / tau) within 1e-12 relative (measured:
    5.3e-14 at tau = 0.05, where the 20-fold exponent amplifies caro_log's few ulp), and the helper's two-action row is
    [1 / S, w / S] with S = 1 + w exactly"""
    rng = np.random.default_rng(5)
    for _ in range(300):
        n, nmax = sorted(int(x) for x in rng.integers(1, 1 << 20, 2))
        if n == nmax:
            continue
        tau = float(rng.choice([0.05, 0.25, 0.5, 1.25, 2.0, 8.0]))
        w = tp.weights(np.array([nmax, n]), tau)
        assert w[0] == 1.0 and 0.0 < w[1] < 1.0
        ref = (n / nmax) ** (1.0 / tau)
        assert abs(w[1] - ref) <= 1e-12 * ref, (n, nmax, tau)
        _, pi = tp.host_policy(np.array([nmax, n]), tau)
        S = np.float64(1.0) + w[1]
        assert pi[0] == np.float64(1.0) / S and pi[1] == w[1] / S


def test_argument_errors():
    L = _lib.load()
    N = np.array([3, 0, 5, 1, 0, 0, 2], np.int32)
    out = np.zeros(7)

    def call(A, n, tau, o=out):
        return L.caro_host_temperature(A, n.ctypes.data if n is not None else None, tau,
                                       o.ctypes.data if o is not None else None)
    assert call(7, N, 0.5) == 2
    for tau in (-1.0, -0.0001, 0.01, 0.049, 8.5, 100.0, float("nan"), float("inf"), float("-inf")):
        assert call(7, N, tau) == -22, tau
        with pytest.raises(ValueError):
            tp.check_tau(tau)
        with pytest.raises(ValueError):
            tp.policy(N, tau)
    for tau in (0.0, 0.05, 1.0, 8.0):
        assert call(7, N, tau) == 2
        assert tp.check_tau(tau) == tau
    assert call(0, N, 1.0) == -22 and call(257, np.zeros(257, np.int32), 0.0, np.zeros(257)) == -22
    assert call(7, None, 1.0) == -22 and call(7, N, 1.0, None) == -22
    assert call(7, np.array([1, -1, 0, 0, 0, 0, 0], np.int32), 1.0) == -22
    assert call(7, np.array([1 << 30, 0, 0, 0, 0, 0, 0], np.int32), 1.0) == -22
    assert call(7, np.full(7, 1 << 28, np.int32), 1.0) == -22  # the sum
    zeros = np.zeros(7, np.int32)
    for tau in (0.05, 0.5, 1.0, 8.0):  # a row without visits has no policy at tau > 0
        assert call(7, zeros, tau) == -22
        with pytest.raises(ValueError):
            tp.policy(zeros, tau)
    assert call(7, zeros, 0.0) == 0 and out.tolist() == [1.0, 0, 0, 0, 0, 0, 0]
    assert tp.policy(zeros, 0.0).tolist() == [1.0, 0, 0, 0, 0, 0, 0]
    with pytest.raises(_lib.CaroError):
        tp.host_policy(zeros, 1.0)


def test_check_triple():
    assert tp.check_triple() == (1.0, 0.0, False) and not tp.is_on(tp.check_triple())
    assert tp.check_triple(0.5, 0.25, True) == (0.5, 0.25, True) and tp.is_on((0.5, 0.25, True))
    assert tp.check_triple(1, 0, 1) == (1.0, 0.0, True) and tp.is_on((1.0, 0.0, True))
    assert tp.is_on((1.0, 0.05, False)) and tp.is_on((0.0, 0.0, False))
    for bad in ((-1, 0, False), (1, 0.01, False), (9, 0, False), (1, float("nan"), False), (1, 0, 2), (1, 0, -1),
                (1, 0, "yes"), (1, 0, None), ("1", 0, False), (True, 0, False), (1, 0, 0.5)):
        with pytest.raises(ValueError):
            tp.check_triple(*bad)


def test_ply_temperatures():
    # sbt0 = 0: every ply is late
    assert tp.ply_temperatures(0, 0, 0.5, 0.25, False) == (0.25, 0.25)
    assert tp.ply_temperatures(7, 0, 0.5, 0.25, True) == (0.25, 1.0)
    # the last early ply and the first late one
    assert tp.ply_temperatures(9, 10, 0.5, 0.25, False) == (0.5, 0.5)
    assert tp.ply_temperatures(10, 10, 0.5, 0.25, False) == (0.25, 0.25)
    assert tp.ply_temperatures(9, 10, 2.0, 0.0, True) == (2.0, 1.0)
    assert tp.ply_temperatures(10, 10, 2.0, 0.0, True) == (0.0, 1.0)
    # the default triple is the engine as it ever was
    assert tp.ply_temperatures(9, 10) == (1.0, 1.0) and tp.ply_temperatures(10, 10) == (0.0, 0.0)
    assert tp.ply_temperatures(0, 0) == (0.0, 0.0)


def test_onehot_share_and_the_eligible_plies_of_early_stop():
    from caro_ai_amd import early_stop as es
    pi = np.array([[0, 1.0, 0], [0.5, 0.5, 0], [0, 0, 1.0], [0.2, 0.3, 0.5]])
    assert tp.onehot_share(pi) == 0.5 and tp.onehot_share(np.zeros((0, 3))) == 0.0
    d = [{"mb": np.array([5, 5, 3, 5, 2]), "games": np.array([[0, 0, 1, 4]])}]  # one game of five plies, last ply first
    assert es.stop_stats(d, 5, 2)["stop_tau0_plies"] == 3
    assert es.stop_stats(d, 5, 2, None, (1.0, 0.0, False)) == es.stop_stats(d, 5, 2)
    assert es.stop_stats(d, 5, 2, None, (1.0, 0.0, True))["stop_tau0_plies"] == 0
    assert es.stop_stats(d, 5, 2, None, (1.0, 0.25, False))["stop_tau0_plies"] == 0
    assert es.stop_stats(d, 5, 2, None, (0.0, 0.5, False))["stop_tau0_plies"] == 2
    assert es.stop_stats(d, 5, 2, None, (0.0, 0.0, False))["stop_tau0_plies"] == 5


def test_library_exports_and_version():
    L = _lib.load()
    assert L.caro_version() == 107
    assert "caro_engine_set_temperature" in _lib.EXPORTS and "caro_host_temperature" in _lib.EXPORTS
