"""The fixed-shape form of the row-Winograd net kernel (k_net_forward_w_c4: connect four's shape as compile-time
constants, one net; csrc/caro_net_kernels.inc, ShapeC4 in csrc/caro_net.hip) against the general form, bit for bit.

Both forms are one source and run the same tiles of the same boards, every output the same fma chain: probs and values
must be EQUAL as raw floats (torch.equal), in dense launches at every tile class and both edges of each, in slot-row
launches, and for the second row range of a launch.  The thresholds between the classes are ncu x TB4 / TB2 / TB of the
device the test runs on; the launch sizes are derived from them.  Which form a launch took is asked of the library
(caro_net_kernel_form, caro_net_last_launch_form), so a case cannot pass by comparing the general form with itself.
The planes are seeded random values of -1 / 0 / +1: the kernels make no use of the planes being stones.
How the slot form is driven follows tests/test_gpu_net_launch_forms.py (rows stated by tests/slot_rows.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import slot_rows as sr
from tests.test_gpu_net import _net
from tests.test_gpu_net_depth import _net as _net_depth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPE, A = (2, 6, 7), 7
FIXED, GENERAL = 0, 1
POOL = 2400  # boards: the largest launch below is ncu * (TB + TB2) + 1 = 2305 on a device of 256 compute units

_S = {}


def _lib():
    from caro_ai_amd import _lib as lib
    return lib


def _hip(key="c4"):
    """one HipNet per net for the whole module (the form is a switch of the handle)"""
    from caro_ai_amd.net_hip import HipNet
    if key not in _S:
        net = {"c4": lambda: _net(SHAPE, A, "best_026_12000.dat"), "c4b": lambda: _net(SHAPE, A, "best_025_10600.dat"),
               "c4k3": lambda: _net_depth(SHAPE, A, 3, seed=3), "f5": lambda: _net((2, 5, 5), 25, None, seed=5)}[key]()
        _S[key] = HipNet(net, DEV, mode="f32w")
        assert _S[key].mode == "f32w1"
    return _S[key]


def _pool():
    if "pool" not in _S:
        g = torch.Generator().manual_seed(4207)
        _S["pool"] = (torch.randint(-1, 2, (POOL,) + SHAPE, generator=g).float()).to(DEV)
    return _S["pool"]


@pytest.fixture(scope="module", autouse=True)
def _close_the_nets():
    yield
    for k, v in list(_S.items()):
        if k != "pool":
            v.close()
    _S.clear()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tiles(hn):
    TB = hn.L.caro_net_boards_per_workgroup(hn.h)
    return (TB,) + sr.split_tile_sizes(hn.H, hn.W, TB)


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dense_sizes():
    """launch sizes at both edges of every tile class, from the device's thresholds: 1, TB -+ 1, and e - 1, e, e + 1 at
    e = ncu x TB4, ncu x TB2 (the 4-way / 2-way limits); ncu x TB (one round of full tiles), + 1, + 64 (overflow in
    4-way tiles); ncu x (TB + TB4) and + 1 (overflow in 2-way tiles); ncu x (TB + TB2) and + 1 (full tiles again)"""
    TB, TB2, TB4 = 6, 3, 1  # asserted against the library in the test
    n = _ncu_static()
    out = [1, TB - 1, TB, TB + 1]
    for e in (n * TB4, n * TB2):
        out += [e - 1, e, e + 1]
    out += [n * TB, n * TB + 1, n * TB + 64, n * (TB + TB4), n * (TB + TB4) + 1, n * (TB + TB2), n * (TB + TB2) + 1]
    return sorted(set(x for x in out if 1 <= x <= POOL))


def _ncu_static():
    """the device's compute units at collection time (256 where there is no device to ask: the ids only)"""
    try:
        return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    except Exception:
        return 256


def _outputs(rows):
    return torch.full((rows, A), -1.0, device=DEV), torch.full((rows,), -9.0, device=DEV)


def _dense(hn, x, form, which=0, c0=0):
    """a dense launch of form `form`: rows [c0, c0 + L) of x with which = 1, all of x with which = 0"""
    hn.set_kernel_form(form)
    assert hn.kernel_form() == form
    rows = x.shape[0]
    counts = torch.tensor([c0, rows - c0] if which else [rows, 0], dtype=torch.int32, device=DEV)
    p, v = _outputs(rows + 8)
    hn.forward_dev(x, counts.data_ptr(), which, rows, p, v, _stream())
    torch.cuda.synchronize()
    assert hn.L.caro_net_last_launch_form(hn.h) == form
    return p, v


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_the_dense_sizes_reach_every_class_and_both_edges():
    hn = _hip()
    TB, TB2, TB4 = _tiles(hn)
    assert (TB, TB2, TB4) == (6, 3, 1)
    n = _ncu()
    sizes = _dense_sizes()
    assert {1, TB - 1, TB, TB + 1, n * TB4 - 1, n * TB4, n * TB4 + 1, n * TB2 - 1, n * TB2, n * TB2 + 1, n * TB,
            n * TB + 1, n * TB + 64} <= set(sizes)
    seen = {sr.tile_class(L, TB, TB2, TB4, n) for L in sizes}
    assert seen == set(sr.CLASSES), seen
    for e, below, above in ((n * TB4, "4-way", "2-way"), (n * TB2, "2-way", "full"), (n * TB, "full", "full+4-way"),
                            (n * (TB + TB4), "full+4-way", "full+2-way"), (n * (TB + TB2), "full+2-way", "full")):
        assert sr.tile_class(e, TB, TB2, TB4, n) == below and sr.tile_class(e + 1, TB, TB2, TB4, n) == above


@pytest.mark.parametrize("L", _dense_sizes())
def test_dense_launch_fixed_form_is_the_general_form(L):
    hn = _hip()
    assert _tiles(hn) == (6, 3, 1)
    x = _pool()[:L].contiguous()
    general = _dense(hn, x, GENERAL)
    fixed = _dense(hn, x, FIXED)
    assert bool((fixed[0][L:] == -1).all()) and bool((fixed[1][L:] == -9).all()), "a row outside the launch was written"
    assert bool((fixed[0][:L].sum(1) - 1).abs().max() < 1e-5)
    assert _same(fixed, general), "L = %d (%s tiles): the fixed-shape form differs from the general form" % (
        L, sr.tile_class(L, *_tiles(hn), _ncu()))


@pytest.mark.parametrize("c0,c1", [(300, 700), (0, 7)])
def test_second_row_range_fixed_form_is_the_general_form(c0, c1):
    """which = 1: rows [counts[0], counts[0] + counts[1])"""
    hn = _hip()
    g = torch.Generator(device=DEV).manual_seed(c0 + c1)
    x = torch.rand((c0 + c1,) + SHAPE, generator=g, device=DEV) * 7.0 + 3.0  # rows below c0: never read
    x[c0:] = _pool()[c0:c0 + c1]
    general = _dense(hn, x, GENERAL, which=1, c0=c0)
    fixed = _dense(hn, x, FIXED, which=1, c0=c0)
    assert bool((fixed[0][:c0] == -1).all()) and bool((fixed[0][c0 + c1:] == -1).all())
    assert _same(fixed, general)


def _slot_launch(hn, form, planes, cnt, B):
    G = len(cnt)
    cls = np.zeros(G, np.int64)
    hn.set_kernel_form(form)
    gp = torch.tensor(sr.gpack(cnt, cls), device=DEV)
    counts = torch.tensor(sr.totals(cnt, cls), dtype=torch.int32, device=DEV)
    p, v = _outputs(G * B)
    _lib().check(hn.L.caro_net_forward_slots(hn.h, None, planes.data_ptr(), counts.data_ptr(), gp.data_ptr(), G, B,
                                             p.data_ptr(), v.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert hn.L.caro_net_last_launch_form(hn.h) == form
    return p, v


def _check_slots(G, B, cnt, want_class):
    hn = _hip()
    cnt = np.asarray(cnt, np.int64)
    cls = np.zeros(G, np.int64)
    rows = sr.game_order_rows(cnt, cls, B, 0)
    L = len(rows)
    assert L == cnt.sum() and sr.tile_class(L, *_tiles(hn), _ncu()) == want_class, (L, want_class)
    g = torch.Generator(device=DEV).manual_seed(G + L)
    planes = torch.rand((G * B,) + SHAPE, generator=g, device=DEV) * 7.0 + 3.0  # rows no launch may read
    rows_t = torch.as_tensor(rows, device=DEV)
    planes[rows_t] = _pool()[:L]
    general = _slot_launch(hn, GENERAL, planes, cnt, B)
    fixed = _slot_launch(hn, FIXED, planes, cnt, B)
    dead = torch.ones(G * B, dtype=torch.bool, device=DEV)
    dead[rows_t] = False
    assert bool((fixed[0][dead] == -1).all()) and bool((fixed[1][dead] == -9).all()), "a row outside the launch was written"
    assert _same(fixed, general), "slot launch of %d leaves (%s): the fixed-shape form differs" % (L, want_class)
    dense = _dense(hn, _pool()[:L].contiguous(), FIXED)  # and both are the dense launch of the leaves in game order
    assert torch.equal(fixed[0][rows_t], dense[0][:L]) and torch.equal(fixed[1][rows_t], dense[1][:L])


def _counts_64(total):
    """64 games, B = 8, the given total; some games at 0 leaves and (where the total allows) some at 8"""
    if total < 16:
        cnt = np.zeros(64, np.int64)
        cnt[37] = total
        return cnt
    cnt = sr.counts_with_total(64, 8, total, seed=total, lead_empty=3, tail_empty=2, full_games=2)
    assert 0 in cnt and 8 in cnt
    return cnt


@pytest.mark.parametrize("what", ["one", "seven", "4-way", "2-way"])
def test_slot_launch_fixed_form_is_the_general_form(what):
    """slot rows, G = 64 games of B = 8: totals 1 and 7, and one total in each tile class that 64 x 8 = 512 rows reach
    (the 4-way class at its upper edge ncu x TB4, the 2-way class 143 boards above its lower edge: 256 and 400 leaves
    on a device of 256 compute units; the classes of larger launches follow below)"""
    hn = _hip()
    tiles, n = _tiles(hn), _ncu()
    total = {"one": 1, "seven": 7, "4-way": min(n * tiles[2], 456), "2-way": n * tiles[2] + 1 + 143}[what]
    klass = what if what in sr.CLASSES else "4-way"
    if total > 456 or sr.tile_class(total, *tiles, n) != klass:
        pytest.skip("64 x 8 rows do not reach the %s class on a device of %d compute units" % (klass, n))
    _check_slots(64, 8, _counts_64(total), klass)


@pytest.mark.parametrize("klass", ["full", "full+4-way", "full+2-way"])
def test_slot_launch_fixed_form_is_the_general_form_large_classes(klass):
    """the classes 512 rows cannot reach: G = 1024 games of B = 8 (the headline's geometry), the smallest launch of the
    class plus 17 boards (a last tile that is not full)"""
    hn = _hip()
    L = sr.pad_to_class(1, klass, *_tiles(hn), _ncu()) + 17
    assert L <= POOL
    _check_slots(1024, 8, sr.counts_with_total(1024, 8, L, seed=L, lead_empty=100, tail_empty=50, full_games=20), klass)


def test_which_launches_take_the_fixed_form():
    """connect four at the reference's depth, one net: fixed; a 5x5 net, a net of three blocks, a which == 2 launch and a
    forced handle: general.  The switch takes 0 and 1 only."""
    c4, c4b, f5, k3 = _hip("c4"), _hip("c4b"), _hip("f5"), _hip("c4k3")
    start = GENERAL if os.environ.get("CARO_NET_KERNEL_FORM") == "1" else FIXED
    assert c4b.kernel_form() == start  # a handle nobody has switched yet
    c4.set_kernel_form(FIXED)
    c4b.set_kernel_form(FIXED)
    assert c4.kernel_form() == FIXED and c4b.kernel_form() == FIXED
    assert f5.kernel_form() == GENERAL and k3.kernel_form() == GENERAL
    for hn, shape in ((f5, (2, 5, 5)), (k3, SHAPE)):
        hn.set_kernel_form(FIXED)  # automatic: still the general kernel
        x = torch.zeros((9,) + shape, device=DEV)
        hn(x)
        torch.cuda.synchronize()
        assert hn.kernel_form() == GENERAL and hn.L.caro_net_last_launch_form(hn.h) == GENERAL
    # both nets of a pair in one launch (which == 2)
    x = _pool()[:300].contiguous()
    counts = torch.tensor([100, 200], dtype=torch.int32, device=DEV)
    p, v = _outputs(300)
    _lib().check(c4.L.caro_net_forward_pair(c4.h, c4b.h, x.data_ptr(), counts.data_ptr(), 300, p.data_ptr(), v.data_ptr(),
                                            _stream()))
    torch.cuda.synchronize()
    assert c4.L.caro_net_last_launch_form(c4.h) == GENERAL and c4.kernel_form() == FIXED
    # ... and its first net's rows are those of that net's own (fixed-form) launch where the tiles are the same ones
    # (300 boards in a pair launch: 2-way tiles of 3 boards, as a one-net launch of 300; net 0 has tiles 0 .. 33 whole)
    tiles, n = _tiles(c4), _ncu()
    if sr.tile_class(300, *tiles, n, pair=True) == sr.tile_class(300, *tiles, n) == "2-way":
        one = _dense(c4, x, FIXED)
        assert torch.equal(p[:99], one[0][:99]) and torch.equal(v[:99], one[1][:99])
    with pytest.raises(_lib().CaroError):
        c4.set_kernel_form(2)
    assert c4.kernel_form() == FIXED
    c4.set_kernel_form(GENERAL)
    assert c4.kernel_form() == GENERAL
    c4.set_kernel_form(FIXED)


def test_the_environment_switch_forces_the_general_form():
    """CARO_NET_KERNEL_FORM=1 when the library is loaded: every net starts forced to the general form (what two runs of
    an unchanged program are alternated with); a fresh process, since the variable is read once"""
    code = ("import torch\n"
            "from tests.test_gpu_net import _net\n"
            "from caro_ai_amd.net_hip import HipNet\n"
            "hn = HipNet(_net((2, 6, 7), 7, 'best_026_12000.dat'), 'cuda:0')\n"
            "a = hn.kernel_form(); hn.set_kernel_form(0); print('forms', a, hn.kernel_form())\n")
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    env = dict(os.environ, CARO_NET_KERNEL_FORM="1")
    out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "forms 1 0" in out.stdout, out.stdout
