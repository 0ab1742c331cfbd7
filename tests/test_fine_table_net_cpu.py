"""The fine grain of the table evaluator (include/caro_hip.h, "Table evaluator", grain 1) on the CPU: the torch twin
(tests/synth_net.py) against the C twin (oracle/caro_oracle.c), the exactness of its float32 values, and the property
it exists for: a float32 sum of its values depends on the order of the terms, which no sum of grain-0 values does."""
import ctypes as C

import numpy as np
import pytest

SALTS = (0, 0x2222, (1 << 64) - 5)


def _oracles():
    from oracle.oracle import Oracle
    return Oracle(Oracle.C4), Oracle(Oracle.MNK, 15, 5)


def _c_eval(o, salt, grain, planes):
    n = planes.shape[0]
    P = np.full((n, o.A), -1, np.float32)
    v = np.full(n, -9, np.float32)
    o.L.oracle_synth_eval_grain(o.h, salt, grain, n, planes.ctypes.data, P.ctypes.data, v.ctypes.data)
    return P, v


def test_fine_grain_twins_agree_and_every_value_is_exact():
    """torch twin == C twin for grain 1 (connect four and 15 x 15, three salts, 17 random boards each); grain 1 is not
    grain 0; grain 0 through the new entry point is the old evaluator; and every P / v is exactly the integer of the
    definition over 2^27 / 2^24 -- the int64 -> float32 conversion of the twins loses nothing at 24 bits."""
    from tests.synth_net import synth_numpy
    rng = np.random.default_rng(0)
    for o in _oracles():
        planes = (rng.random((17, 2, o.rows, o.cols)) < 0.3).astype(np.float32)
        o.L.oracle_synth_eval.argtypes = [C.c_void_p, C.c_uint64, C.c_int] + [C.c_void_p] * 3
        for salt in SALTS:
            P1, v1 = synth_numpy(planes, o.A, salt, grain=1)
            Pc, vc = _c_eval(o, salt, 1, planes)
            assert P1.dtype == np.float32 and v1.dtype == np.float32
            assert np.array_equal(P1.view(np.uint32), Pc.view(np.uint32))
            assert np.array_equal(v1.view(np.uint32), vc.view(np.uint32))
            # grain 0: the three ways to ask for it give the same bits, and they are not grain 1's
            P0, v0 = synth_numpy(planes, o.A, salt)
            Pg, vg = _c_eval(o, salt, 0, planes)
            Po, vo = np.zeros_like(Pg), np.zeros_like(vg)
            o.L.oracle_synth_eval(o.h, salt, 17, planes.ctypes.data, Po.ctypes.data, vo.ctypes.data)
            assert np.array_equal(P0, Pg) and np.array_equal(v0, vg) and np.array_equal(P0, Po) and np.array_equal(v0, vo)
            assert not np.array_equal(P0, P1) and not np.array_equal(v0, v1)
            # the round trip through the stated integer, in float64 (which holds every float32 exactly)
            mp = P1.astype(np.float64) * 2.0 ** 27
            mv = v1.astype(np.float64) * 2.0 ** 24
            assert np.array_equal(mp, np.rint(mp)) and mp.min() >= 1 and mp.max() <= 2 ** 24
            assert np.array_equal(mv, np.rint(mv)) and np.abs(mv).max() <= 2 ** 24 - 1
            assert np.array_equal((mp.astype(np.int64).astype(np.float32) / np.float32(2.0 ** 27)).view(np.uint32),
                                  P1.view(np.uint32))
            assert np.array_equal((mv.astype(np.int64).astype(np.float32) / np.float32(2.0 ** 24)).view(np.uint32),
                                  v1.view(np.uint32))
            assert P1.max() <= 0.125 and P1.min() > 0 and np.abs(v1).max() < 1
            # the values use the mantissa: more than the 11 bits of grain 0 in nearly every one
            assert (mv.astype(np.int64) % 8192 != 0).mean() > 0.9 and (mp.astype(np.int64) % 8192 != 0).mean() > 0.9


def test_oracle_search_takes_the_grain():
    """Oracle.use_synth_net(grain=1) searches with the fine values: the root's priors are grain 1's of the root planes"""
    from oracle.oracle import Oracle
    from tests.synth_net import synth_numpy
    o = Oracle(Oracle.C4)
    s = o.initial_state
    planes = o.states_to_training_batch([s], [0])
    for grain, salt in ((0, 0), (1, 0), (1, 0x2222)):
        o.clear()
        o.use_synth_net(salt, grain=grain)
        o.set_stream(3, 0)
        o.search_batch(2, 8, s, 0)
        want = synth_numpy(planes, o.A, salt, grain)[0][0]
        assert np.array_equal(o.get_node(s)["P"], want), (grain, salt)


def _non_associative_share(x):
    a, b, c = (x[k::3].astype(np.float32) for k in range(3))
    return float(((a + b) + c != a + (b + c)).mean())


@pytest.mark.parametrize("what", ["v", "P"])
def test_float32_sums_of_fine_values_depend_on_their_order(what):
    """A condition on the evaluator, not on any kernel: over the values of 3 000 random connect-four boards (seed 7,
    30 % of the cells set) taken as 1 000 triples, (a + b) + c != a + (b + c) in float32 for at least 10 % of the
    triples at grain 1 and for none at grain 0.  The hash's own share, measured before the seed was fixed (seeds 0 .. 9 gave 12.8 .. 16.3 % for v, 15.5 .. 20.2 % for P[0]): with this
    seed 14.8 % for v (the values a backup adds into W; uniform 24-bit triples give 14.8 % too) and 17.2 % for the first
    prior P[0]; grain 0: 0 % for both."""
    from tests.synth_net import synth_numpy
    rng = np.random.default_rng(7)
    planes = (rng.random((3000, 2, 6, 7)) < 0.3).astype(np.float32)
    share = {}
    for grain in (0, 1):
        P, v = synth_numpy(planes, 7, 0, grain)
        share[grain] = _non_associative_share(v if what == "v" else P[:, 0])
    print("non-associative float32 triples of %s: grain 0 %.1f %%, grain 1 %.1f %%" % (what, 100 * share[0], 100 * share[1]))
    assert share[0] == 0.0
    assert share[1] >= 0.10
