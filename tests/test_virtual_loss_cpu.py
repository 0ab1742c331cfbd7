"""Virtual loss without a GPU (include/caro_hip.h, "virtual loss"): the host helper caro_host_vl_level -- built from
the function the kernels call -- against the numpy statement of the rule (caro_ai_amd/virtual_loss.py) on random rows, bit
for bit; counts of zero against caro_host_fpu_level at reduction 0; hand-built rows; the error codes; the exports and the
version; check_n; the train CLI's option."""
import ctypes as C

import numpy as np
import pytest

from caro_ai_amd import _lib
from caro_ai_amd import fpu
from caro_ai_amd import virtual_loss as vl

EXPLORE, C_PUCT = 0.25, 1.0
SIZES = (7, 9, 36, 81, 225)


def _row(rng, A):
    """one random row: visit counts with many zeros (sometimes all), strong and non-strong edges, a partly illegal mask,
    and counts of the rule up to 8 on a few actions"""
    N = (rng.integers(0, 40, A) * (rng.random(A) < rng.choice([0.1, 0.5, 0.9]))).astype(np.int32)
    if rng.random() < 0.1:
        N[:] = 0
    strong = (rng.random(A) < 0.5).astype(np.int32)
    val = rng.uniform(-1.0, 1.0, A)
    W = (val * N).astype(np.float32)
    Q = np.where(N > 0, val + rng.normal(0, 1e-3, A), 0.0).astype(np.float32)
    P = rng.dirichlet(np.full(A, 0.5)).astype(np.float32)
    legal = (rng.random(A) < rng.choice([0.6, 1.0])).astype(np.uint8)
    if not legal.any():
        legal[rng.integers(A)] = 1
    noise = rng.dirichlet(np.full(A, 0.3))
    c = (rng.integers(1, 9, A) * (rng.random(A) < rng.choice([0.0, 0.05, 0.3]))).astype(np.int32)
    return dict(N=N, W=W, Q=Q, P=P, strong=strong, legal=legal, noise=noise, c=c)


def _args(root, r, n_vl, c=None):
    return (root, r["N"], r["W"], r["Q"], r["P"], r["strong"], r["legal"], r["noise"] if root else None, C_PUCT, EXPLORE,
            r["c"] if c is None else c, n_vl)


def _same_bits(root, scores, want):
    if root:
        assert want.dtype == np.float64
        return np.array_equal(scores.view(np.uint64), want.view(np.uint64))
    assert want.dtype == np.float32
    got32 = scores.astype(np.float32)
    return (np.array_equal(got32.astype(np.float64).view(np.uint64), scores.view(np.uint64))  # widened float32
            and np.array_equal(got32.view(np.uint32), want.view(np.uint32)))


@pytest.mark.parametrize("A", SIZES)
def test_host_level_equals_the_numpy_rule_bit_for_bit(A):
    rng = np.random.default_rng(20261019 + A)
    moved = {True: 0, False: 0}
    lost = 0
    for i in range(2000):
        r = _row(rng, A)
        root = bool(i & 1)
        n_vl = int(rng.choice([0, 1, 2, 3, 4, 16]))
        choice, scores = vl.host_level(*_args(root, r, n_vl))
        want = vl.level_scores(*_args(root, r, n_vl))
        assert _same_bits(root, scores, want), (i, A, root, n_vl)
        assert choice == vl.level_choice(*_args(root, r, n_vl)) == int(np.argmax(want)), (i, A, root, n_vl)
        off = int(np.argmax(vl.level_scores(*_args(root, r, 0))))
        moved[root] += choice != off
        lost += bool(n_vl and ((r["N"] == 0) & (r["c"] > 0) & (r["legal"] != 0)).any())
    assert moved[True] > 20 and moved[False] > 20  # the rule moved choices at both kinds of level
    assert lost > 20  # rows with a virtual visit on an edge without a real one


def test_zero_counts_are_the_level_without_the_feature():
    rng = np.random.default_rng(7)
    for i in range(1500):
        r = _row(rng, SIZES[i % len(SIZES)])
        root = bool(i & 1)
        base_c, base = fpu.host_level(root, r["N"], r["W"], r["Q"], r["P"], r["strong"], r["legal"],
                                      r["noise"] if root else None, C_PUCT, EXPLORE, 0.0, 0.0)
        for n_vl, c in ((2, np.zeros_like(r["c"])), (0, r["c"])):
            choice, scores = vl.host_level(*_args(root, r, n_vl, c))
            assert choice == base_c
            assert np.array_equal(scores.view(np.uint64), base.view(np.uint64)), (i, root, n_vl)


def test_hand_built_rows():
    # two equal unvisited actions: the first descent takes the lower one, the second -- which sees that edge with one
    # virtual visit, lost -- takes the other
    for root in (False, True):
        r = dict(N=np.zeros(2, np.int32), W=np.zeros(2, np.float32), Q=np.zeros(2, np.float32),
                 P=np.full(2, 0.5, np.float32), strong=np.zeros(2, np.int32), legal=np.ones(2, np.uint8),
                 noise=np.full(2, 0.5), c=np.zeros(2, np.int32))
        # (a row without visits has a U term of 0 -- sqrt(0): one real visit elsewhere would be another node; give the row
        # a visited third action instead)
        r = {k: np.concatenate([x, x[:1]]) for k, x in r.items()}
        r["N"][2], r["W"][2], r["Q"][2], r["P"][2] = 4, -2.0, -0.5, 0.0
        first, _ = vl.host_level(*_args(root, r, 2))
        assert first == 0
        r["c"][first] = 1
        second, sc = vl.host_level(*_args(root, r, 2))
        assert second == 1 and vl.level_choice(*_args(root, r, 2)) == 1
        # an edge with N = 0 and c = 1: Q' = (0 * 0 - v) / (0 + v) = -1, U over 1 + v with nsum' = 4 + v
        for n_vl in (1, 2, 16):
            _, sc = vl.host_level(*_args(root, r, n_vl))
            if root:
                prob = np.float64(np.float32(0.75) * np.float32(0.5)) + 0.25 * 0.5
                assert sc[0] == -1.0 + (prob * np.sqrt(np.float64(4 + n_vl))) / np.float64(1 + n_vl)
            else:
                u = (np.float32(0.5) * np.float32(np.sqrt(np.float64(4 + n_vl)))) / np.float32(1 + n_vl)
                assert np.float32(sc[0]) == np.float32(-1.0) + u
    # a visited edge: Q' = (q0 * N - v) / (N + v) in the level's precision
    r = dict(N=np.array([3, 5], np.int32), W=np.array([1.5, -1.0], np.float32), Q=np.array([0.5, -0.2], np.float32),
             P=np.array([0.5, 0.5], np.float32), strong=np.zeros(2, np.int32), legal=np.ones(2, np.uint8),
             noise=np.full(2, 0.5), c=np.array([2, 0], np.int32))
    _, sc = vl.host_level(*_args(False, r, 3))
    q = (np.float32(0.5) * np.float32(3) - np.float32(6)) / np.float32(9)
    assert np.float32(sc[0]) == q + (np.float32(0.5) * np.float32(np.sqrt(np.float64(14)))) / np.float32(10)
    assert np.float32(sc[1]) == np.float32(-0.2) + (np.float32(0.5) * np.float32(np.sqrt(np.float64(14)))) / np.float32(6)
    _, sc = vl.host_level(*_args(True, r, 3))
    assert sc[0] == ((np.float64(np.float32(1.5)) / 3.0) * 3.0 - 6.0) / 9.0 + (0.5 * np.sqrt(np.float64(14))) / 10.0


def test_minibatch_choices_replays_the_descents_in_order():
    # one node, four unvisited equal actions and no children in the tree: four descents take four different actions with
    # the rule, and all the same one without it
    row = dict(N=np.array([0, 0, 0, 0, 6], np.int32), W=np.array([0, 0, 0, 0, -3.0], np.float32),
               Q=np.array([0, 0, 0, 0, -0.5], np.float32), P=np.array([0.25, 0.25, 0.25, 0.25, 0.0], np.float32),
               strong=np.zeros(5, np.int32))
    kw = dict(row_of=lambda k: row if k == "root" else None, legal_of=lambda k: np.ones(5, bool),
              child_of=lambda k, a: ((k, a), False), root_key="root", noise=np.full((4, 5), 0.2), c_puct=C_PUCT,
              explore=EXPLORE)
    on = vl.minibatch_choices(4, n_vl=2, **kw)
    off = vl.minibatch_choices(4, n_vl=0, **kw)
    assert [p[0][1] for p in on] == [0, 1, 2, 3] and [p[0][1] for p in off] == [0, 0, 0, 0]
    assert all(len(p) == 1 for p in on)


def test_error_codes_exports_and_version():
    L = _lib.load()
    assert L.caro_version() >= 106
    for name in ("caro_engine_set_virtual_loss", "caro_host_vl_level"):
        assert hasattr(L, name) and name in _lib._SIGNATURES
    r = _row(np.random.default_rng(1), 7)

    def call(A, n_vl, root=0, noise=True, c=None, N=None, drop=None):
        out = np.zeros(256, np.float64)
        a = {k: np.resize(r[k], 256) for k in r}
        if c is not None:
            a["c"] = np.resize(np.asarray(c, np.int32), 256)
        if N is not None:
            a["N"] = np.resize(np.asarray(N, np.int32), 256)
        ptr = {k: (None if k == drop else x.ctypes.data) for k, x in a.items()}
        return L.caro_host_vl_level(A, root, ptr["N"], ptr["W"], ptr["Q"], ptr["P"], ptr["strong"], ptr["legal"],
                                    ptr["noise"] if noise else None, C_PUCT, EXPLORE, ptr["c"], n_vl, out.ctypes.data)

    assert call(7, 2) >= 0 and call(256, 16) >= 0 and call(1, 0) >= 0 and call(7, 2, root=1) >= 0
    for n_vl in (-1, 17, 1 << 20):
        assert call(7, n_vl) == -22
    for A in (0, -1, 257):
        assert call(A, 2) == -22
    assert call(7, 2, root=1, noise=False) == -22
    assert call(7, 2, root=0, noise=False) >= 0  # (a level below the root needs no noise row)
    assert call(7, 2, c=[-1]) == -22 and call(7, 2, c=[65]) == -22
    assert call(7, 2, N=[-1]) == -22 and call(7, 2, N=[1 << 24]) == -22
    assert call(7, 16, N=[(1 << 24) // 7 - 8], c=[64]) == -22  # the sum of N' is out of range
    for drop in ("N", "W", "Q", "P", "strong", "legal", "c"):
        assert call(7, 2, drop=drop) == -22
    assert L.caro_engine_set_virtual_loss(None, 2) == -22


def test_check_n():
    assert [vl.check_n(n) for n in (0, 1, 16, np.int32(3))] == [0, 1, 16, 3]
    for bad in (-1, 17, 2.0, "2", None, True, float("nan")):
        with pytest.raises(ValueError):
            vl.check_n(bad)


def test_cli_option_parses_and_exits_on_a_bad_value():
    from caro_ai_amd import train
    base = ["-n", "r", "-g", "0"]
    a = train.parse_args(base)
    assert a.virtual_loss is None and train.virtual_loss_from_args(a) is None
    assert train.virtual_loss_from_args(train.parse_args(base + ["--virtual-loss", "2"])) == 2
    assert train.virtual_loss_from_args(train.parse_args(base + ["--virtual-loss", "0"])) == 0
    for bad in ("17", "-1"):
        with pytest.raises(SystemExit) as e:
            train.virtual_loss_from_args(train.parse_args(base + ["--virtual-loss", bad]))
        assert "--virtual-loss" in str(e.value)
    with pytest.raises(SystemExit):
        train.parse_args(base + ["--virtual-loss", "2.5"])
