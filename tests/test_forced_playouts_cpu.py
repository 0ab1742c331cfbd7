"""Forced playouts and policy target pruning on the host (include/caro_hip.h, "forced playouts"): the two host helpers,
compiled from the functions the kernels call, against the plain numpy statement of the rules
(caro_ai_amd/forced_playouts.py); hand-built rows; argument errors; the exports; the train CLI's flag."""
import ctypes as C
import re

import numpy as np
import pytest

from caro_ai_amd import _lib
from caro_ai_amd import forced_playouts as fp

EXPLORE = 0.25
SIZES = (7, 9, 36, 81, 225)


def _rows(A, n, seed):
    """n random root rows: N in 0 .. 60 with many zeros, ones and twos; P a softmax; Q in [-1, 1]; a Dirichlet-like
    noise row; about one action in ten illegal (its N is 0, as in a tree)"""
    rng = np.random.default_rng(seed)
    pool = np.array([0] * 12 + [1] * 8 + [2] * 6 + list(range(3, 61)))
    for _ in range(n):
        legal = rng.random(A) < 0.9
        legal[rng.integers(A)] = True
        N = rng.choice(pool, size=A).astype(np.int32) * legal
        if N.sum() == 0:
            N[np.flatnonzero(legal)[0]] = 1 + rng.integers(5)
        x = rng.normal(size=A) * 2.0
        P = (np.exp(x) / np.exp(x).sum()).astype(np.float32)
        Q = rng.uniform(-1.0, 1.0, A)
        g = rng.gamma(0.3, size=A) + 1e-300
        yield N, P, Q, g / g.sum(), legal


@pytest.mark.parametrize("A", SIZES)
def test_host_helpers_equal_the_numpy_rules(A):
    forced_rows = pruned_rows = dropped_ones = 0
    for i, (N, P, Q, nz, legal) in enumerate(_rows(A, 2000, 100 + A)):
        k = (0.5, 2.0, 5.0, 64.0)[i % 4]
        c = (1.0, 0.3, 4.0)[i % 3]
        got, count = fp.host_forced_root(N, P, nz, legal, EXPLORE, k)
        want = fp.forced_root(N, P, nz, legal, EXPLORE, k)
        np.testing.assert_array_equal(got, want, err_msg="forced, row %d" % i)
        assert count == int(want.sum())
        n2, b = fp.host_forced_prune(N, Q, P, c, k)
        w2, wb = fp.prune(N, Q, P, c, k)
        np.testing.assert_array_equal(n2, w2, err_msg="pruned, row %d" % i)
        assert b == wb == int(np.argmax(N)) and n2[b] == N[b] and n2.sum() > 0
        assert (n2 <= N).all() and (n2 >= 0).all() and not (n2 == 1)[np.arange(A) != b].any()
        forced_rows += bool(want.any())
        pruned_rows += int(n2.sum() < N.sum())
        dropped_ones += int(((N == 1) & (n2 == 0)).sum())
    assert forced_rows > 200 and pruned_rows > 200 and dropped_ones > 200  # the rows exercise both rules


def test_nothing_is_forced_at_k_zero_and_a_zero_visit_child_never():
    N = np.array([5, 0, 1, 3, 0, 2, 7], np.int32)
    P = np.array([.1, .4, .2, .05, .05, .1, .1], np.float32)
    nz = np.array([.0, .9, .02, .02, .02, .02, .02])
    legal = np.ones(7, bool)
    assert fp.host_forced_root(N, P, nz, legal, EXPLORE, 0.0) == (pytest.approx(np.zeros(7, bool)), 0)
    f, count = fp.host_forced_root(N, P, nz, legal, EXPLORE, 64.0)
    assert not f[1] and not f[4] and count == 5  # the unvisited children, however large their prior or k
    np.testing.assert_array_equal(f, fp.forced_root(N, P, nz, legal, EXPLORE, 64.0))


def test_the_lowest_forced_action_wins_and_an_illegal_one_is_never_forced():
    N = np.array([9, 1, 1, 1, 0, 0, 0], np.int32)
    P = np.full(7, 1.0 / 7, np.float32)
    nz = np.full(7, 1.0 / 7)
    legal = np.array([1, 0, 1, 1, 1, 1, 1], bool)
    f, count = fp.host_forced_root(N, P, nz, legal, EXPLORE, 2.0)
    # prob = 1/7, T = 12: 1 < 2 * 12 / 7 for the one-visit children, 81 > 3.4 for the leader; action 1 is illegal
    assert f.tolist() == [False, False, True, True, False, False, False] and count == 2
    assert fp.root_choice(N, P, nz, legal, EXPLORE, 2.0, off_action=0) == 2
    assert fp.root_choice(N, P, nz, legal, EXPLORE, 0.0, off_action=5) == 5


def test_the_forcing_threshold_is_strict():
    # n * n < (k * prob) * T with prob = 0.5 exactly (P = 0.5, noise = 0.5, explore = 0.25), k = 2, T = 16: 16 < 16 fails
    N = np.array([4, 12], np.int32)
    P = np.array([0.5, 0.5], np.float32)
    nz = np.array([0.5, 0.5])
    assert fp.host_forced_root(N, P, nz, [1, 1], EXPLORE, 2.0)[0].tolist() == [False, False]
    assert fp.host_forced_root(N + np.array([-1, 1], np.int32), P, nz, [1, 1], EXPLORE, 2.0)[0].tolist() == [True, False]


def test_a_child_reduced_to_one_visit_becomes_zero():
    # b = 0 with S* = 0.5 + 0.5 * 4 / 11 = 0.6818; child 1: Q = 0, P = 0.25, N = 3, F = int(sqrt(2 * 0.25 * 16)) = 2,
    # scores at n = 1, 2, 3: 0.5, 0.333, 0.25 -- all below S*, so the smallest n in [1, 3] is 1, which becomes 0
    N = np.array([10, 3, 3], np.int32)
    Q = np.array([0.5, 0.0, 0.9])
    P = np.array([0.5, 0.25, 0.25], np.float32)
    n2, b = fp.host_forced_prune(N, Q, P, 1.0, 2.0)
    assert b == 0 and n2.tolist() == [10, 0, 3]  # child 2: 0.9 + 0.25 > S* even at N = 3: whole
    np.testing.assert_array_equal(n2, fp.prune(N, Q, P, 1.0, 2.0)[0])


def test_the_best_child_is_never_reduced_and_a_row_that_fails_the_predicate_stays_whole():
    # every other child scores above S* even with all its visits: nothing is taken (no child has exactly one visit)
    N = np.array([4, 9, 3, 2], np.int32)
    Q = np.array([0.9, -0.5, 0.8, 0.95])
    P = np.array([0.25, 0.25, 0.25, 0.25], np.float32)
    n2, b = fp.host_forced_prune(N, Q, P, 1.0, 64.0)
    assert b == 1 and n2.tolist() == N.tolist()
    # the best child keeps its visits however bad its Q; the others may lose theirs
    N = np.array([2, 30, 5], np.int32)
    Q = np.array([-1.0, -1.0, -1.0])
    n2, b = fp.host_forced_prune(N, Q, P[:3], 1.0, 64.0)
    assert b == 1 and n2[1] == 30 and n2.sum() > 0
    # the first maximum is b
    n2, b = fp.host_forced_prune(np.array([7, 7, 1], np.int32), np.zeros(3), P[:3], 1.0, 2.0)
    assert b == 0 and n2[0] == 7


def test_k_zero_prunes_only_what_the_predicate_gives_without_forced_visits():
    # F = 0: the range is [N, N], so a child stays whole unless it has one visit (rule 4)
    N = np.array([10, 4, 1], np.int32)
    n2, _ = fp.host_forced_prune(N, np.zeros(3), np.array([.5, .3, .2], np.float32), 1.0, 0.0)
    assert n2.tolist() == [10, 4, 0]


def test_argument_errors():
    L = _lib.load()
    N = np.array([1, 2, 3], np.int32)
    P = np.array([.2, .3, .5], np.float32)
    Q = np.zeros(3)
    nz = np.array([.2, .3, .5])
    legal = np.ones(3, np.uint8)
    out8, out32 = np.zeros(3, np.uint8), np.zeros(3, np.int32)
    p = lambda a: a.ctypes.data
    for k in (-1.0, 64.5, float("nan"), float("inf")):
        assert L.caro_host_forced_root(3, p(N), p(P), p(nz), p(legal), EXPLORE, k, p(out8)) == -22
        assert L.caro_host_forced_prune(3, p(N), p(Q), p(P), 1.0, k, p(out32)) == -22
        assert L.caro_last_error()
        with pytest.raises(ValueError):
            fp.check_k(k)
    for A in (0, -1, 257):
        assert L.caro_host_forced_root(A, p(N), p(P), p(nz), p(legal), EXPLORE, 2.0, p(out8)) == -22
        assert L.caro_host_forced_prune(A, p(N), p(Q), p(P), 1.0, 2.0, p(out32)) == -22
    assert L.caro_host_forced_root(3, None, p(P), p(nz), p(legal), EXPLORE, 2.0, p(out8)) == -22
    assert L.caro_host_forced_prune(3, p(N), p(Q), p(P), 1.0, 2.0, None) == -22
    neg = np.array([1, -2, 3], np.int32)
    assert L.caro_host_forced_root(3, p(neg), p(P), p(nz), p(legal), EXPLORE, 2.0, p(out8)) == -22
    assert L.caro_host_forced_prune(3, p(neg), p(Q), p(P), 1.0, 2.0, p(out32)) == -22
    zero = np.zeros(3, np.int32)
    assert L.caro_host_forced_prune(3, p(zero), p(Q), p(P), 1.0, 2.0, p(out32)) == -22  # no visits: no policy
    assert L.caro_host_forced_root(3, p(zero), p(P), p(nz), p(legal), EXPLORE, 2.0, p(out8)) == 0
    with pytest.raises(_lib.CaroError):
        fp.host_forced_prune(zero, Q, P, 1.0, 2.0)
    with pytest.raises(ValueError):
        fp.prune(zero, Q, P, 1.0, 2.0)
    assert L.caro_engine_set_forced_playouts(None, 2.0) == -22
    assert L.caro_forced_stats(None, None, None) == -22
    assert fp.check_k(0) == 0.0 and fp.check_k(2) == 2.0 and fp.check_k(64) == 64.0
    for bad in (True, "x", None):
        with pytest.raises(ValueError):
            fp.check_k(bad)


def test_exports_and_binding_table():
    import os
    L = _lib.load()
    names = ("caro_engine_set_forced_playouts", "caro_forced_stats", "caro_host_forced_root", "caro_host_forced_prune")
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "caro_hip.h")).read()
    for name in names:
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert re.search(r"\b%s\s*\(" % name, hdr)
    assert L.caro_version() >= 103
    assert _lib._SIGNATURES["caro_engine_set_forced_playouts"] == (C.c_int, [C.c_void_p, C.c_double])
    assert _lib._SIGNATURES["caro_forced_stats"] == (C.c_int, [C.c_void_p] * 3)
    assert len(_lib._SIGNATURES["caro_host_forced_root"][1]) == 8 and len(_lib._SIGNATURES["caro_host_forced_prune"][1]) == 7
    assert "forced playouts" in hdr and "open_dev;\n} caro_drain_extra;" in hdr  # the rule is stated; the struct did not grow
    assert fp.STAT_NAMES == ("root_descents", "forced_descents", "pruned_plies", "visits_removed")


def test_entropy_and_shares():
    assert fp.entropy([[1.0, 0.0], [0.5, 0.5]]).tolist() == [0.0, pytest.approx(np.log(2.0))]
    st = dict(zip(fp.STAT_NAMES, (100, 7, 3, 12)), forced_share=0.07)
    assert fp.shares(st, 400) == {"forced_share": 0.07, "pruned_visits_share": 0.03}
    assert fp.shares(dict(st, forced_share=0.0), 0)["pruned_visits_share"] == 0.0


def test_train_cli_parses_the_flag_and_refuses_a_bad_k():
    from caro_ai_amd import train
    assert train.parse_args(["-n", "r", "-g", "0"]).forced_playouts is None
    assert train.parse_args(["-n", "r", "-g", "0", "--forced-playouts", "2"]).forced_playouts == 2.0
    for bad in ("-1", "65", "nan"):
        with pytest.raises(SystemExit, match="--forced-playouts"):
            train.main(["-n", "r", "-g", "0", "--forced-playouts", bad])
