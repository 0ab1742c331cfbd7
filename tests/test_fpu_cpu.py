"""First-play urgency reduction without a GPU (include/caro_hip.h, "first-play urgency"): the host helper
caro_host_fpu_level -- built from the functions the kernels call -- against the numpy statement of the rule
(caro_ai_amd/fpu.py) on random rows, bit for bit; reduction 0 against a plain restatement of today's formula; two
hand-built rows; the error codes; the version; the train CLI's two options."""
import math

import numpy as np
import pytest

from caro_ai_amd import _lib
from caro_ai_amd import fpu

EXPLORE, C_PUCT = 0.25, 1.0
SIZES = (7, 9, 16, 64, 81, 225)


def _row(rng, A):
    """one random row: visit counts with many zeros, strong and non-strong edges, a partly illegal mask, and priors that
    include 0, 1 and subnormals"""
    N = rng.integers(0, 40, A) * (rng.random(A) < rng.choice([0.1, 0.5, 0.9]))
    N = N.astype(np.int32)
    if rng.random() < 0.1:
        N[:] = 0
    strong = (rng.random(A) < 0.5).astype(np.int32)
    val = rng.uniform(-1.0, 1.0, A)
    W = (val * N).astype(np.float32)
    Q = np.where(N > 0, val + rng.normal(0, 1e-3, A), 0.0).astype(np.float32)
    P = rng.dirichlet(np.full(A, 0.5)).astype(np.float32)
    special = rng.random(A)
    P[special < 0.05] = 0.0
    P[(special >= 0.05) & (special < 0.08)] = 1.0
    P[(special >= 0.08) & (special < 0.12)] = np.float32(1e-42)  # subnormal
    P[(special >= 0.12) & (special < 0.14)] = np.float32(2.0 ** -23)  # below one unit of the mass
    legal = (rng.random(A) < rng.choice([0.6, 1.0])).astype(np.uint8)
    if not legal.any():
        legal[rng.integers(A)] = 1
    noise = rng.dirichlet(np.full(A, 0.3))
    return dict(N=N, W=W, Q=Q, P=P, strong=strong, legal=legal, noise=noise)


def _today(root, r, q_up=0.0):
    """today's level in plain numpy (lib/mcts.py:79-84 and the root's noised float64 form), no word of the feature"""
    N = r["N"].astype(np.int64)
    legal = r["legal"].astype(bool)
    if root:
        Wd = r["W"].astype(np.float64)
        qd = np.where(r["strong"] != 0, r["Q"].astype(np.float64), np.where(N > 0, Wd / np.maximum(N, 1), 0.0))
        prob = (np.float32(1.0 - EXPLORE) * r["P"]).astype(np.float64) + EXPLORE * r["noise"]
        sc = qd + ((np.float64(np.float32(C_PUCT)) * prob) * np.float64(math.sqrt(int(N.sum())))) / (1 + N)
        return np.where(legal, sc, -np.inf)
    tt = np.float32(C_PUCT) * r["P"]
    tt = tt * np.float32(math.sqrt(int(N.sum())))
    tt = tt / (1 + N).astype(np.float32)
    return np.where(legal, r["Q"] + tt, np.float32(-np.inf)).astype(np.float32)


def _args(root, r, q_up, red):
    return (root, r["N"], r["W"], r["Q"], r["P"], r["strong"], r["legal"], r["noise"] if root else None, C_PUCT, EXPLORE,
            q_up, red)


def test_host_level_equals_the_numpy_rule_bit_for_bit():
    rng = np.random.default_rng(20261019)
    differ = {True: 0, False: 0}
    for i in range(3000):
        A = SIZES[i % len(SIZES)]
        r = _row(rng, A)
        root = bool(i & 1)
        q_up = np.float32(rng.uniform(-1, 1)) if rng.random() < 0.9 else np.float32(0.0)
        red = float(rng.choice([0.0, 0.25, 0.5, 1.0, 2.0, rng.uniform(0, 2)]))
        choice, scores = fpu.host_level(*_args(root, r, q_up, red))
        want = fpu.level_scores(*_args(root, r, q_up, red))
        if root:
            assert want.dtype == np.float64
            assert np.array_equal(scores.view(np.uint64), want.view(np.uint64)), (i, A, red)
        else:
            assert want.dtype == np.float32
            got32 = scores.astype(np.float32)
            assert np.array_equal(got32.astype(np.float64).view(np.uint64), scores.view(np.uint64))  # widened float32
            assert np.array_equal(got32.view(np.uint32), want.view(np.uint32)), (i, A, red)
        assert choice == fpu.level_choice(*_args(root, r, q_up, red)) == int(np.argmax(want)), (i, A, red)
        differ[root] += choice != int(np.argmax(_today(root, r)))
    assert differ[True] > 50 and differ[False] > 50  # the rule moved choices at both kinds of level


def test_reduction_zero_is_todays_formula():
    rng = np.random.default_rng(7)
    for i in range(1200):
        r = _row(rng, SIZES[i % len(SIZES)])
        root = bool(i & 1)
        choice, scores = fpu.host_level(*_args(root, r, np.float32(rng.uniform(-1, 1)), 0.0))
        want = _today(root, r)
        assert choice == int(np.argmax(want))
        if root:
            assert np.array_equal(scores.view(np.uint64), want.view(np.uint64))
        else:
            assert np.array_equal(scores.astype(np.float32).view(np.uint32), want.view(np.uint32))


def test_visited_mass_is_an_integer_sum():
    P = np.array([0.5, 1.0, 0.0, 1e-42, 2.0 ** -22, 0.25, 3.0, -1.0], np.float32)
    N = np.array([1, 2, 3, 4, 5, 0, 1, 1], np.int32)
    legal = np.array([1, 1, 1, 1, 1, 1, 1, 0], np.uint8)
    # 0.5 -> 2^21, 1 -> 2^22, 0 and the subnormal -> 0, 2^-22 -> 1, an unvisited action and an illegal one: nothing,
    # 3.0 clamps to 1
    assert fpu.visited_mass(N, P, legal) == (1 << 21) + (1 << 22) + 1 + (1 << 22)
    assert fpu.visited_sqrt(1 << 22) == 1.0 and fpu.visited_sqrt(0) == 0.0


def test_hand_built_rows():
    # a losing node below the root: both visited children have Q < 0, the third one is unvisited.  today its 0 + u beats
    # them; with the rule its Q is -q_up - r * s, s from the visited mass
    N = np.array([60, 30, 0], np.int32)
    Q = np.array([-0.4, -0.5, 0.0], np.float32)
    W = (Q * N).astype(np.float32)
    P = np.array([0.48, 0.48, 0.04], np.float32)
    r = dict(N=N, W=W, Q=Q, P=P, strong=np.ones(3, np.int32), legal=np.ones(3, np.uint8), noise=np.full(3, 1 / 3))
    off, _ = fpu.host_level(*_args(False, r, np.float32(0.5), 0.0))
    on, sc = fpu.host_level(*_args(False, r, np.float32(0.5), 0.5))
    assert off == 2 and on == 0
    m = 2 * int(np.float32(0.48) * np.float32(4194304.0))
    s_vis = math.sqrt(m / 4194304.0)
    q = np.float32(np.float64(np.float32(-0.5)) - 0.5 * s_vis)
    assert np.float32(sc[2]) == q + (np.float32(0.04) * np.float32(math.sqrt(90))) / np.float32(1.0)
    assert fpu.level_choice(*_args(False, r, np.float32(0.5), 0.0)) == 2
    assert fpu.level_choice(*_args(False, r, np.float32(0.5), 0.5)) == 0
    # a winning node: the visited child is ahead either way, the two rules agree
    r2 = dict(r, Q=np.array([0.6, 0.1, 0.0], np.float32), W=np.array([36.0, 3.0, 0.0], np.float32))
    for root in (False, True):
        a0, _ = fpu.host_level(*_args(root, r2, np.float32(-0.5), 0.0))
        a1, _ = fpu.host_level(*_args(root, r2, np.float32(-0.5), 0.5))
        assert a0 == a1 == (2 if root else 0)  # (the root's noised prior makes the unvisited child's U the largest)
    # the root level takes its base from the row: the first maximum of N is action 0, its Q -0.4
    a, sc = fpu.host_level(*_args(True, r, np.float32(0.9), 0.25))
    prob2 = np.float64(np.float32(0.75) * np.float32(0.04)) + 0.25 * (1 / 3)
    assert sc[2] == (np.float64(np.float32(-0.4)) - 0.25 * s_vis) + (prob2 * math.sqrt(90)) / 1.0
    # a row without visits: base 0 and s 0, nothing changes
    r3 = dict(r, N=np.zeros(3, np.int32), W=np.zeros(3, np.float32), Q=np.zeros(3, np.float32))
    assert np.array_equal(fpu.host_level(*_args(True, r3, np.float32(0), 0.5))[1],
                          fpu.host_level(*_args(True, r3, np.float32(0), 0.0))[1])


def test_error_codes_and_version():
    L = _lib.load()
    assert L.caro_version() >= 105
    r = _row(np.random.default_rng(1), 7)

    def call(A, red, root=0, noise=True):
        out = np.zeros(256, np.float64)
        N, W, Q, P = (np.resize(r[k], 256) for k in ("N", "W", "Q", "P"))
        strong, legal, nz = np.resize(r["strong"], 256), np.resize(r["legal"], 256), np.resize(r["noise"], 256)
        return L.caro_host_fpu_level(A, root, N.ctypes.data, W.ctypes.data, Q.ctypes.data, P.ctypes.data,
                                     strong.ctypes.data, legal.ctypes.data, nz.ctypes.data if noise else None, C_PUCT,
                                     EXPLORE, 0.0, red, out.ctypes.data)

    assert call(7, 0.5) >= 0 and call(256, 2.0) >= 0 and call(1, 0.0) >= 0
    for red in (float("nan"), -0.1, 2.5, float("inf")):
        assert call(7, red) == -22
    for A in (0, -1, 257):
        assert call(A, 0.5) == -22
    assert call(7, 0.5, root=1, noise=False) == -22
    for bad in (float("nan"), -1, 2.01, "x", True):
        with pytest.raises(ValueError):
            fpu.check_reduction(bad)
    assert fpu.check_pair(0.5) == (0.5, 0.5) and fpu.check_pair((0.5, 0.25)) == (0.5, 0.25)
    assert fpu.check_pair((0.5, None)) == (0.5, 0.5)


def test_cli_options_parse():
    from caro_ai_amd import train
    base = ["-n", "r", "-g", "0"]
    a = train.parse_args(base)
    assert a.fpu_reduction is None and a.fpu_root_reduction is None and train.fpu_from_args(a) is None
    assert train.fpu_from_args(train.parse_args(base + ["--fpu-reduction", "0.5"])) == (0.5, 0.5)
    a = train.parse_args(base + ["--fpu-reduction", "0.5", "--fpu-root-reduction", "0.25"])
    assert train.fpu_from_args(a) == (0.5, 0.25)
    for bad in (["--fpu-reduction", "3"], ["--fpu-reduction", "0.5", "--fpu-root-reduction", "-1"],
                ["--fpu-root-reduction", "0.25"], ["--fpu-reduction", "nan"]):
        with pytest.raises(SystemExit):
            train.fpu_from_args(train.parse_args(base + bad))
