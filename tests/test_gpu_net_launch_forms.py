"""The launch forms of the HIP net against its dense single-net launch, bit for bit.

tests/test_gpu_net.py gates the dense launch of one net (HipNet.__call__) against torch.  Every launch of the engine's hot
path takes another form: slot rows (caro_net_forward_slots / _slot_list: game g's j-th leaf at row g * B + j, every
workgroup rebuilding its dense tile from the games' leaf counts -- tile_rows / tile_rows_pre of csrc/caro_net.hip), two
nets in one launch (caro_net_forward_pair / _pair_at), or the second row range of a launch (which = 1).  Each of them
runs the tiles of a dense launch of the same boards in the same order, so it must return THE SAME BITS; which rows those
are is stated independently of the kernels in tests/slot_rows.py.  Every output buffer starts as a sentinel (-1 for P,
-9 for v) that the rows outside the launch must keep, every plane row outside the launch holds garbage, and the live
rows of every case also pass the torch gate of tests/test_gpu_net.py.

Each case of (a) states the games per thread (ceil(G / 512); above 4 the kernels take the plain tile_rows) and the tile
class it was written for, and asserts both."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import slot_rows as sr
from tests.test_gpu_net import _boards, _net
from tests.test_gpu_net_depth import _net as _net_depth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NCU = 256  # compute units of the device the launch sizes below are written for

# net key -> (planes shape, actions, how to make it, residual blocks)
NETS = {
    "c4": ((2, 6, 7), 7, lambda: _net((2, 6, 7), 7, "best_026_12000.dat"), 5),
    "c4b": ((2, 6, 7), 7, lambda: _net((2, 6, 7), 7, "best_025_10600.dat"), 5),
    "c4k3": ((2, 6, 7), 7, lambda: _net_depth((2, 6, 7), 7, 3, seed=3), 3),
    "c4k10": ((2, 6, 7), 7, lambda: _net_depth((2, 6, 7), 7, 10, seed=10), 10),
    "t3": ((2, 3, 3), 9, lambda: _net((2, 3, 3), 9, "best_005_00900.dat"), 5),
    "f5": ((2, 5, 5), 25, lambda: _net((2, 5, 5), 25, None, seed=5), 5),
    "f5b": ((2, 5, 5), 25, lambda: _net((2, 5, 5), 25, None, seed=55), 5),
    "g15": ((2, 15, 15), 225, lambda: _net((2, 15, 15), 225, None, seed=15), 5),
    "g15b": ((2, 15, 15), 225, lambda: _net((2, 15, 15), 225, None, seed=65), 5),
    "g12": ((2, 12, 12), 144, lambda: _net((2, 12, 12), 144, None, seed=12), 5),
}
POOL = {(6, 7): 3100, (3, 3): 7936, (5, 5): 3072, (15, 15): 400, (12, 12): 400}  # boards per board size


class _Ref:
    """a net, its pool of boards and -- computed when first asked for, once per board -- torch's float32 forward of them
    on the CPU (float64 as well for a net deeper than five blocks)"""

    def __init__(self, key):
        self.shape, self.A, make, self.depth = NETS[key]
        self.net = make()
        self.x = _pool(self.shape)
        n = len(self.x)
        self.have = np.zeros(n, bool)
        self.p = torch.zeros((n, self.A))
        self.v = torch.zeros(n)
        self.p64 = torch.zeros((n, self.A), dtype=torch.float64)
        self.v64 = torch.zeros(n, dtype=torch.float64)

    def rows(self, idx):
        idx = np.asarray(idx)
        new = np.unique(idx[~self.have[idx]])
        if len(new):
            todo = torch.as_tensor(new)
            x = self.x[todo]
            with torch.no_grad():
                lg, vl = self.net(x)
                self.p[todo], self.v[todo] = torch.softmax(lg, dim=1), vl[:, 0]
                if self.depth > 5:
                    lg64, vl64 = self.net.double()(x.double())
                    self.p64[todo], self.v64[todo] = torch.softmax(lg64, dim=1), vl64[:, 0]
                    self.net.float()
            self.have[new] = True
        return torch.as_tensor(idx)


_POOLS, _REFS, _HIPNETS = {}, {}, {}


def _pool(shape):
    """the boards of every case of a board size: the k-th board a launch serves is pool board k (CPU and device copy)"""
    shape = tuple(shape)
    if shape not in _POOLS:
        x = _boards(POOL[shape[1:]], shape, 4242 + shape[1])
        _POOLS[shape] = (x, x.to(DEV))
    return _POOLS[shape][0]


def _pool_dev(shape):
    _pool(shape)
    return _POOLS[tuple(shape)][1]


def _ref(key):
    if key not in _REFS:
        _REFS[key] = _Ref(key)
    return _REFS[key]


def _hip(key, mode):
    """one HipNet per (net, mode) for the whole module"""
    from caro_ai_amd.net_hip import HipNet
    if (key, mode) not in _HIPNETS:
        hn = HipNet(_ref(key).net, DEV, mode=mode)
        hn.key = key
        _HIPNETS[(key, mode)] = hn
    return _HIPNETS[(key, mode)]


@pytest.fixture(scope="module", autouse=True)
def _close_the_nets():
    yield
    for hn in _HIPNETS.values():
        hn.close()
    _HIPNETS.clear()
    _REFS.clear()
    _POOLS.clear()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from caro_ai_amd import _lib as lib
    return lib


def _tiles(hn):
    """(TB, TB2, TB4) of the net's kernel: split tiles exist in the row-Winograd form only"""
    H, W = hn.H, hn.W
    TB = hn.L.caro_net_boards_per_workgroup(hn.h)
    want = min(255 // (H * W), 32)
    if hn.mode == "f32w1":
        want = min(want, 128 // (-(-H // 2) * W))
    elif hn.mode == "f32w2":
        want = 1
    assert TB == want, (hn.mode, H, W, TB, want)
    return (TB,) + (sr.split_tile_sizes(H, W, TB) if hn.mode == "f32w1" else (0, 0))


def _ncu():
    n = torch.cuda.get_device_properties(0).multi_processor_count
    assert n == NCU, "the launch sizes of this module are written for a device of %d compute units, this one has %d" % (NCU, n)
    return n


def _class(hn, L, pair=False):
    return sr.tile_class(L, *_tiles(hn), _ncu(), pair=pair)


def _garbage(rows, shape, seed):
    """plane rows no launch may read: neither zeros nor stones"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.rand((rows,) + shape, generator=g, device=DEV) * 7.0 + 3.0


def _outputs(rows, A):
    return torch.full((rows, A), -1.0, device=DEV), torch.full((rows,), -9.0, device=DEV)


def _untouched(p, v, live):
    """every row outside `live` still holds its sentinel"""
    dead = torch.ones(p.shape[0], dtype=torch.bool, device=p.device)
    if len(live):
        dead[torch.as_tensor(np.asarray(live), device=p.device)] = False
    return bool((p[dead] == -1).all()) and bool((v[dead] == -9).all())


def _gate(key, pool_idx, p, v, launch_rows):
    """(e): the rows p, v (board k = pool board pool_idx[k] through net `key`) against torch on the CPU -- at most 1 600 of
    them, the first and last 800.  |dP| < 1e-4 (3e-4 in a launch of more than 1 000 boards), |dv| < 1e-4, sum P = 1
    within 1e-5; a net deeper than five blocks instead: no further from a float64 forward than max(4 x torch-float32's
    own distance, 1e-6), priors and values."""
    n = len(pool_idx)
    if n == 0:
        return
    pick = np.arange(n) if n <= 1600 else np.r_[0:800, n - 800:n]
    ref = _ref(key)
    idx = ref.rows(np.asarray(pool_idx)[pick])
    sel = torch.as_tensor(pick, device=p.device)
    ph, vh = p[sel].cpu(), v[sel].cpu()
    dp, dv = (ph - ref.p[idx]).abs().max().item(), (vh - ref.v[idx]).abs().max().item()
    ds = (ph.sum(1) - 1).abs().max().item()
    print("  gate %s: %d of %d boards, launch of %d: |dP|=%.3e |dv|=%.3e |sum P - 1|=%.3e" % (key, len(pick), n, launch_rows,
                                                                                         dp, dv, ds))
    assert ds <= 1e-5, ds
    if ref.depth > 5:
        e_hip, e_ref = (ph.double() - ref.p64[idx]).abs().max().item(), (ref.p[idx].double() - ref.p64[idx]).abs().max().item()
        ev_hip, ev_ref = (vh.double() - ref.v64[idx]).abs().max().item(), (ref.v[idx].double() - ref.v64[idx]).abs().max().item()
        print("  gate %s (depth %d): e_hip64=%.3e e_torch64=%.3e ev_hip64=%.3e ev_torch64=%.3e"
              % (key, ref.depth, e_hip, e_ref, ev_hip, ev_ref))
        assert e_hip < max(4 * e_ref, 1e-6), (e_hip, e_ref)
        assert ev_hip < max(4 * ev_ref, 1e-6), (ev_hip, ev_ref)
    else:
        assert dp < (3e-4 if launch_rows > 1000 else 1e-4), dp
        assert dv < 1e-4, dv


_NO_LIST = object()


def _slot_launch(n0, n1, planes, cnt, cls, B, slist=_NO_LIST):
    """caro_net_forward_slots, or with `slist` (None or an int32[2][G * B] array) caro_net_forward_slot_list"""
    G = len(cnt)
    gp = torch.tensor(sr.gpack(cnt, cls), device=DEV)
    counts = torch.tensor(sr.totals(cnt, cls), dtype=torch.int32, device=DEV)
    p, v = _outputs(G * B, n0.A)
    assert planes.shape[0] == G * B and planes.is_contiguous()
    L = n0.L
    if slist is _NO_LIST:
        rc = L.caro_net_forward_slots(n0.h, n1.h if n1 else None, planes.data_ptr(), counts.data_ptr(), gp.data_ptr(), G, B,
                                      p.data_ptr(), v.data_ptr(), _stream())
    else:
        sl = None if slist is None else torch.tensor(np.ascontiguousarray(slist, np.int32), device=DEV)
        assert sl is None or sl.shape == (2, G * B)
        rc = L.caro_net_forward_slot_list(n0.h, n1.h if n1 else None, planes.data_ptr(), counts.data_ptr(), gp.data_ptr(),
                                          None if sl is None else sl.data_ptr(), G, B, p.data_ptr(), v.data_ptr(), _stream())
    _lib().check(rc)
    torch.cuda.synchronize()
    return p, v


def _pair_launch(n0, n1, x, l0, l1, row1_base=None, spare=8):
    """caro_net_forward_pair (row1_base None) / _pair_at over the rows of x, max_rows = l0 + l1 exactly; the outputs have
    x's rows and `spare` more"""
    counts = torch.tensor([l0, l1], dtype=torch.int32, device=DEV)
    p, v = _outputs(x.shape[0] + spare, n0.A)
    L = n0.L
    if row1_base is None:
        rc = L.caro_net_forward_pair(n0.h, n1.h, x.data_ptr(), counts.data_ptr(), l0 + l1, p.data_ptr(), v.data_ptr(), _stream())
    else:
        rc = L.caro_net_forward_pair_at(n0.h, n1.h, x.data_ptr(), counts.data_ptr(), row1_base, l0 + l1, p.data_ptr(),
                                        v.data_ptr(), _stream())
    _lib().check(rc)
    torch.cuda.synchronize()
    return p, v


def _dense(hn, x):
    p, v = hn(x.contiguous())
    torch.cuda.synchronize()
    return p, v


def _drawn(spec):
    return len(spec) == 2 and isinstance(spec[1], dict)


def _counts(G, B, spec):
    """spec: a tuple of counts, or (L, {counts_with_total's keywords})"""
    if _drawn(spec):
        return sr.counts_with_total(G, B, spec[0], seed=1000 * G + spec[0], **spec[1])
    cnt = np.asarray(spec, np.int64)
    assert len(cnt) == G and cnt.max() <= B
    return cnt


# ---- (a) one net: slot launch == dense launch of the rows gathered in game order -------------------------------------

def _check_slots_one_net(hn, G, B, cnt, want_gpt, want_class):
    shape = _ref(hn.key).shape
    cls = np.zeros(G, np.int64)
    rows = sr.game_order_rows(cnt, cls, B, 0)
    L = len(rows)
    assert sr.games_per_thread(G) == want_gpt and L == cnt.sum()
    if L:
        assert _class(hn, L) == want_class, (L, _class(hn, L), want_class)
    planes = _garbage(G * B, shape, G + B)
    rows_t = torch.as_tensor(rows, device=DEV)
    planes[rows_t] = _pool_dev(shape)[:L]
    p, v = _slot_launch(hn, None, planes, cnt, cls, B)
    assert _untouched(p, v, rows), "a row outside the launch was written"
    if L == 0:
        return None
    pd, vd = _dense(hn, _pool_dev(shape)[:L])
    bad = (~((p[rows_t] == pd).all(1) & (v[rows_t] == vd))).nonzero().flatten().tolist()
    assert not bad, "%d of %d leaves differ from the dense launch, the first at dense index %d (slot row %d)" % (
        len(bad), L, bad[0], rows[bad[0]])
    _gate(hn.key, np.arange(L), pd, vd, L)
    return p, v


# G, B, counts, games per thread, tile class of the row-Winograd form on connect four
C4_CASES = [
    (1, 1, (0,), 1, None),                       # nothing is written anywhere and nothing fails
    (1, 1, (1,), 1, "4-way"),
    (1, 8, (8,), 1, "4-way"),
    (3, 255, (255, 0, 254), 1, "2-way"),         # one game across ~43 tiles, the whole 8-bit count field, an empty game between
    (512, 2, (200, {}), 1, "4-way"),
    (513, 2, (700, {}), 2, "2-way"),
    (1024, 8, (1500, dict(lead_empty=300, tail_empty=100, full_games=20)), 2, "full"),   # the headline's shape
    (1024, 8, (1700, {}), 2, "full+4-way"),
    (1024, 8, (2000, {}), 2, "full+2-way"),
    (1024, 8, (3100, {}), 2, "full"),            # two rounds of full tiles
    (1025, 1, (257, {}), 3, "2-way"),
    (2048, 1, (768, {}), 4, "2-way"),
    (2049, 1, (769, {}), 5, "full"),             # 5 games per thread and up: the plain tile_rows
    (2049, 2, (40, dict(lead_empty=2029)), 5, "4-way"),   # every leaf in the last 20 games (all of them full)
    (2049, 2, (20, dict(lead_empty=2039)), 5, "4-way"),   # ... in the last 10
    (4096, 1, (1537, {}), 8, "full+4-way"),
]
C4_SUBSET = [c for c in C4_CASES if (c[0], c[2][0]) in ((3, 255), (513, 700), (1024, 1500), (2049, 769), (2049, 40))]
assert len(C4_SUBSET) == 5


def _case_id(c):
    return "G%d-B%d-L%d" % (c[0], c[1], c[2][0] if _drawn(c[2]) else sum(c[2]))


def test_the_case_table_covers_what_it_is_meant_to():
    """1, 2, 3 and 4 games per thread and the plain map; all five tile classes; counts 0 and 255; L = 0"""
    assert {c[3] for c in C4_CASES} >= {1, 2, 3, 4, 5}
    assert {c[4] for c in C4_CASES} == set(sr.CLASSES) | {None}
    assert any(0 in c[2] and 255 in c[2] for c in C4_CASES if not _drawn(c[2]))


@pytest.mark.parametrize("case", C4_CASES, ids=_case_id)
def test_slot_launch_is_the_dense_launch_connect_four(case):
    """(a) the default form (row Winograd: tile_rows_pre up to four games per thread, tile_rows above) on 6x7"""
    G, B, spec, gpt, klass = case
    hn = _hip("c4", "f32w")
    assert hn.mode == "f32w1" and _tiles(hn) == (6, 3, 1)
    _check_slots_one_net(hn, G, B, _counts(G, B, spec), gpt, klass)


@pytest.mark.parametrize("case", C4_SUBSET, ids=_case_id)
@pytest.mark.parametrize("key,mode", [("c4", "f32"), ("c4", "bf16x3"), ("c4k3", "f32w")])
def test_slot_launch_is_the_dense_launch_other_kernels(key, mode, case):
    """(a) the direct kernel and bf16x3 (plain tile_rows at every G, full tiles only) and a net of three blocks in the
    row-Winograd form (the run-time-depth instantiation)"""
    G, B, spec, gpt, klass = case
    hn = _hip(key, mode)
    assert hn.depth == (3 if key == "c4k3" else 5)
    _check_slots_one_net(hn, G, B, _counts(G, B, spec), gpt, klass if hn.mode == "f32w1" else "full")


@pytest.mark.parametrize("G", [1024, 2049])
@pytest.mark.parametrize("key,tiles", [("t3", (21, 10, 5)), ("f5", (8, 4, 2))])
def test_slot_launch_is_the_dense_launch_other_tile_sizes(key, tiles, G):
    """(a) 3x3 and 5x5 in the row-Winograd form: other boards per tile; the largest launch of each tile class"""
    hn = _hip(key, "f32w")
    assert hn.mode == "f32w1" and _tiles(hn) == tiles
    for klass in sr.CLASSES:
        L = sr.largest_of_class(klass, *tiles, _ncu())
        B = -(-L // G) + 1
        _check_slots_one_net(hn, G, B, sr.counts_with_total(G, B, L, seed=G + L), sr.games_per_thread(G), klass)


# large boards, one per workgroup, the heads of the launch in k_net_heads (32 boards per workgroup): L % 32 = 0, 5, 31, 1
BIG_CASES = [
    (1, 32, (32,), 1),
    (3, 255, (255, 0, 70), 1),
    (513, 2, (95, {}), 2),
    (2048, 1, (96, {}), 4),
    (2049, 1, (257, {}), 5),
]


@pytest.mark.parametrize("case", BIG_CASES, ids=_case_id)
@pytest.mark.parametrize("key,mode", [("g15", "f32w2"), ("g12", "f32w2"), ("g15", "bf16x3")])
def test_slot_launch_is_the_dense_launch_large_boards(key, mode, case):
    """(a) 15x15 and 12x12 in the 2-D Winograd form, 15x15 in bf16x3"""
    G, B, spec, gpt = case
    hn = _hip(key, mode)
    assert _tiles(hn) == (1, 0, 0)
    _check_slots_one_net(hn, G, B, _counts(G, B, spec), gpt, "full")


# ---- (b) two nets: slot launch == dense pair launch of class 0's rows, then class 1's --------------------------------

def _classes(G, pattern, seed):
    if pattern == "random":
        return np.random.default_rng(seed).integers(0, 2, G)
    return {"all-0": np.zeros(G, np.int64), "all-1": np.ones(G, np.int64), "alternating": np.arange(G) % 2}[pattern]


def _check_slots_two_nets(n0, n1, G, B, cnt, cls, slist=_NO_LIST):
    shape = _ref(n0.key).shape
    rows = np.concatenate([sr.game_order_rows(cnt, cls, B, 0), sr.game_order_rows(cnt, cls, B, 1)])
    l0, l1 = sr.totals(cnt, cls)
    L = l0 + l1
    assert L == len(rows) == cnt.sum()
    planes = _garbage(G * B, shape, G + B + 1)
    rows_t = torch.as_tensor(rows, device=DEV)
    planes[rows_t] = _pool_dev(shape)[:L]
    p, v = _slot_launch(n0, n1, planes, cnt, cls, B, slist)
    assert _untouched(p, v, rows), "a row outside the launch was written"
    if L == 0:
        return
    pd, vd = _pair_launch(n0, n1, _pool_dev(shape)[:L].contiguous(), l0, l1)
    assert _untouched(pd, vd, np.arange(L))
    bad = (~((p[rows_t] == pd[:L]).all(1) & (v[rows_t] == vd[:L]))).nonzero().flatten().tolist()
    assert not bad, "%d of %d leaves (%d + %d) differ from the dense pair launch, the first at dense index %d (slot row %d)" % (
        len(bad), L, l0, l1, bad[0], rows[bad[0]])
    _gate(n0.key, np.arange(l0), pd[:l0], vd[:l0], L)
    _gate(n1.key, np.arange(l0, L), pd[l0:L], vd[l0:L], L)


@pytest.mark.parametrize("case", C4_CASES, ids=_case_id)
def test_two_net_slot_launch_is_the_dense_pair_launch(case):
    """(b) the shipped pair in the default form, every geometry of (a), a random class per game"""
    G, B, spec = case[:3]
    _check_slots_two_nets(_hip("c4", "f32w"), _hip("c4b", "f32w"), G, B, _counts(G, B, spec), _classes(G, "random", G + B))


@pytest.mark.parametrize("pattern", ["all-0", "all-1", "alternating"])
@pytest.mark.parametrize("mode", ["f32w", "f32"])
def test_two_net_slot_launch_class_patterns(mode, pattern):
    """(b) every game of one class -- the other net's part of the launch is empty -- and classes in turn"""
    for G, B, spec in [c[:3] for c in C4_SUBSET]:
        _check_slots_two_nets(_hip("c4", mode), _hip("c4b", mode), G, B, _counts(G, B, spec), _classes(G, pattern, 0))


@pytest.mark.parametrize("total", [255, 256, 765, 766, 1500])
@pytest.mark.parametrize("mode", ["f32w", "f32"])
def test_two_net_slot_launch_at_the_pair_thresholds(mode, total):
    """(b) L0 + L1 on both sides of the two-net class rule (4-way up to 255 boards, 2-way up to 765 on connect four), the
    first class ending on a tile's last board, its first and its last but one"""
    n0, n1 = _hip("c4", mode), _hip("c4b", mode)
    klass = _class(n0, total, pair=True)
    assert klass == ({255: "4-way", 256: "2-way", 765: "2-way", 766: "full", 1500: "full"}[total] if mode == "f32w" else "full")
    cap = sr.boards_per_tile(klass, *_tiles(n0))[0]
    G, B = 1024, 8
    base = (total // 3) // cap * cap
    for l0 in sorted({base, base + 1, base + cap - 1}):
        assert l0 % cap in (0, 1, cap - 1)
        cls = _classes(G, "random", total + l0)
        cnt = np.zeros(G, np.int64)
        cnt[cls == 0] = sr.counts_with_total(int((cls == 0).sum()), B, l0, seed=l0)
        cnt[cls == 1] = sr.counts_with_total(int((cls == 1).sum()), B, total - l0, seed=total)
        _check_slots_two_nets(n0, n1, G, B, cnt, cls)


@pytest.mark.parametrize("order", ["5-10", "10-5"])
def test_two_net_slot_launch_of_a_5_and_a_10_block_net(order):
    """(b) nets of unequal depth in one slot launch (the run-time-depth kernels) against their dense pair launch"""
    a, b = _hip("c4", "f32w"), _hip("c4k10", "f32w")
    n0, n1 = (a, b) if order == "5-10" else (b, a)
    for G, B, spec in [c[:3] for c in C4_SUBSET]:
        _check_slots_two_nets(n0, n1, G, B, _counts(G, B, spec), _classes(G, "random", G))


@pytest.mark.parametrize("l0", [0, 31, 32, 33])
def test_two_net_slot_launch_on_15x15(l0):
    """(b) one board per workgroup, the heads of each net in workgroups of 32 boards: the first net's share around 32"""
    n0, n1 = _hip("g15", "f32w2"), _hip("g15b", "f32w2")
    G, B, l1 = 513, 2, 45
    cls = _classes(G, "random", 15 + l0)
    cnt = np.zeros(G, np.int64)
    cnt[cls == 0] = sr.counts_with_total(int((cls == 0).sum()), B, l0, seed=l0)
    cnt[cls == 1] = sr.counts_with_total(int((cls == 1).sum()), B, l1, seed=l1)
    _check_slots_two_nets(n0, n1, G, B, cnt, cls)


# ---- (c) the slot list -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G,B,L", [(2049, 1, 257), (64, 8, 200)])
def test_slot_list_on_15x15(G, B, L):
    """(c) the form that reads the list (2-D Winograd): the leaves listed in a shuffled order come back with the bits of
    the dense launches, one net and two"""
    n0, n1 = _hip("g15", "f32w2"), _hip("g15b", "f32w2")
    assert n0.L.caro_net_uses_slot_list(n0.h) == 1
    cnt = sr.counts_with_total(G, B, L, seed=G)
    shape = _ref("g15").shape
    rng = np.random.default_rng(G)
    # one net
    cls = np.zeros(G, np.int64)
    rows = sr.game_order_rows(cnt, cls, B, 0)
    sl = sr.slot_list(cnt, cls, B, rng)
    assert sl[0, :L].tolist() != rows.tolist()
    planes = _garbage(G * B, shape, G)
    rows_t = torch.as_tensor(rows, device=DEV)
    planes[rows_t] = _pool_dev(shape)[:L]
    p, v = _slot_launch(n0, None, planes, cnt, cls, B, slist=sl)
    pd, vd = _dense(n0, _pool_dev(shape)[:L])
    assert _untouched(p, v, rows)
    assert torch.equal(p[rows_t], pd) and torch.equal(v[rows_t], vd)
    p0, v0 = _slot_launch(n0, None, planes, cnt, cls, B, slist=None)   # a NULL list: the game-order map
    assert torch.equal(p0, p) and torch.equal(v0, v)
    # two nets
    cls = _classes(G, "random", G)
    _check_slots_two_nets(n0, n1, G, B, cnt, cls, slist=sr.slot_list(cnt, cls, B, rng))


@pytest.mark.parametrize("two", [False, True])
def test_slot_list_is_ignored_where_tiles_hold_several_boards(two):
    """(c) the header's promise for every other form: a list that names the wrong rows changes nothing on connect four"""
    n0, n1 = _hip("c4", "f32w"), (_hip("c4b", "f32w") if two else None)
    assert n0.L.caro_net_uses_slot_list(n0.h) == 0
    G, B, L = 1024, 8, 1500
    shape = _ref("c4").shape
    cnt = sr.counts_with_total(G, B, L, seed=3)
    cls = _classes(G, "random", 3) if two else np.zeros(G, np.int64)
    rows = np.concatenate([sr.game_order_rows(cnt, cls, B, 0), sr.game_order_rows(cnt, cls, B, 1)])
    planes = _garbage(G * B, shape, 3)
    planes[torch.as_tensor(rows, device=DEV)] = _pool_dev(shape)[:L]
    wrong = np.zeros((2, G * B), np.int32)                      # every leaf "at row 0" ...
    wrong[:, 1::2] = np.arange(G * B, dtype=np.int32)[::-1][1::2]  # ... or at rows counted from the end
    p, v = _slot_launch(n0, n1, planes, cnt, cls, B)
    pw, vw = _slot_launch(n0, n1, planes, cnt, cls, B, slist=wrong)
    assert torch.equal(p, pw) and torch.equal(v, vw)
    assert _untouched(pw, vw, rows)


# ---- (d) dense pair forms at the class boundaries --------------------------------------------------------------------

def _single_reference(hn, x, klass):
    """the rows of x through ONE net in a dense launch of tile class `klass`: x padded with other boards up to the
    smallest launch of that class"""
    n = x.shape[0]
    Lp = sr.pad_to_class(n, klass, *_tiles(hn), _ncu())
    assert Lp is not None and Lp - n <= len(_pool_dev(x.shape[1:]))
    pool = _pool_dev(x.shape[1:])
    xs = torch.cat([x, pool[len(pool) - (Lp - n):]]) if Lp > n else x
    assert _class(hn, xs.shape[0]) == klass
    p, v = _dense(hn, xs)
    return p[:n], v[:n]


def _check_dense_pair(n0, n1, l0, l1, want_class=None):
    shape = _ref(n0.key).shape
    L = l0 + l1
    x = _pool_dev(shape)[:L].contiguous()
    klass = _class(n0, L, pair=True)
    assert want_class is None or klass == want_class, (L, klass, want_class)
    p, v = _pair_launch(n0, n1, x, l0, l1)
    assert _untouched(p, v, np.arange(L))
    cap = sr.boards_per_tile(klass, *_tiles(n0))[0]
    for hn, lo, n in ((n0, 0, l0), (n1, l0, l1)):
        whole = n // cap * cap   # the tiles the pair launch fills; the last, partial one has the torch gate only
        if whole:
            ps, vs = _single_reference(hn, x[lo:lo + whole], klass)
            bad = (~((p[lo:lo + whole] == ps).all(1) & (v[lo:lo + whole] == vs))).nonzero().flatten().tolist()
            assert not bad, "pair (%d, %d), %s tiles: %d rows of net %s differ from its single launch, the first at %d" % (
                l0, l1, klass, len(bad), hn.key, lo + bad[0])
        _gate(hn.key, np.arange(lo, lo + n), p[lo:lo + n], v[lo:lo + n], L)
    return p, v


@pytest.mark.parametrize("total,klass", [(255, "4-way"), (256, "2-way"), (765, "2-way"), (766, "full"), (1535, "full"),
                                         (1700, "full")])
def test_dense_pair_launch_at_the_class_boundaries(total, klass):
    """(d) caro_net_forward_pair on connect four, max_rows = L0 + L1 exactly: each net's whole tiles carry the bits of
    that net's own dense launch of the same tile class, in an even and in a skewed split"""
    n0, n1 = _hip("c4", "f32w"), _hip("c4b", "f32w")
    for l0 in (total // 2, total - 10, 7):
        _check_dense_pair(n0, n1, l0, total - l0, klass)


@pytest.mark.parametrize("l0,l1,klass", [(255, 255, "4-way"), (509, 511, "2-way"), (1, 509, "4-way"), (257, 255, "2-way")])
def test_dense_pair_launch_fills_its_grid_on_5x5(l0, l1, klass):
    """(d) 5x5 (tiles of 8 / 4 / 2 boards): both classes round up to a tile of their own -- L0 = 1 and L1 = TB4 - 1 modulo
    TB4 at the largest 4-way sum, likewise modulo TB2 -- and the launch has exactly the workgroups it needs"""
    n0, n1 = _hip("f5", "f32w"), _hip("f5b", "f32w")
    assert _tiles(n0) == (8, 4, 2)
    cap = sr.boards_per_tile(klass, 8, 4, 2)[0]
    assert l0 % cap == 1 and l1 % cap == cap - 1
    _check_dense_pair(n0, n1, l0, l1, klass)


@pytest.mark.parametrize("key0,key1,mode,l0,l1", [("c4", "c4b", "f32w", 100, 155), ("c4", "c4b", "f32w", 300, 400),
                                                   ("c4", "c4b", "f32w", 900, 800), ("c4", "c4b", "f32", 100, 155),
                                                   ("c4", "c4k10", "f32w", 300, 400), ("g15", "g15b", "f32w2", 31, 33)])
def test_pair_at_moves_the_second_nets_rows(key0, key1, mode, l0, l1):
    """(d) caro_net_forward_pair_at: row1_base = L0 + 37 gives the second net's rows of caro_net_forward_pair 37 rows
    further down and leaves the gap alone; row1_base = -1 is caro_net_forward_pair"""
    n0, n1 = _hip(key0, mode), _hip(key1, mode)
    shape = _ref(key0).shape
    L, gap = l0 + l1, 37
    pool = _pool_dev(shape)
    p, v = _pair_launch(n0, n1, pool[:L].contiguous(), l0, l1)
    pm, vm = _pair_launch(n0, n1, pool[:L].contiguous(), l0, l1, row1_base=-1)
    assert torch.equal(p, pm) and torch.equal(v, vm)
    x = _garbage(L + gap, shape, L)
    x[:l0] = pool[:l0]
    x[l0 + gap:] = pool[l0:L]
    pa, va = _pair_launch(n0, n1, x, l0, l1, row1_base=l0 + gap)
    assert _untouched(pa, va, np.r_[0:l0, l0 + gap:L + gap])
    assert torch.equal(pa[:l0], p[:l0]) and torch.equal(va[:l0], v[:l0])
    assert torch.equal(pa[l0 + gap:L + gap], p[l0:L]) and torch.equal(va[l0 + gap:L + gap], v[l0:L])
    _gate(key0, np.arange(l0), p[:l0], v[:l0], L)
    _gate(key1, np.arange(l0, L), p[l0:L], v[l0:L], L)


@pytest.mark.parametrize("c0,c1", [(1500, 300), (0, 7)])
@pytest.mark.parametrize("mode", ["f32w", "f32", "bf16x3"])
def test_second_row_range_of_a_launch(mode, c0, c1):
    """(d) caro_net_forward with which = 1: rows [counts[0], counts[0] + counts[1]) carry the bits of a which = 0 launch of
    those boards (the same L, so the same tiles), everything else keeps its sentinel"""
    hn = _hip("c4", mode)
    shape = _ref("c4").shape
    L = c0 + c1
    x = _garbage(L, shape, L)
    x[c0:] = _pool_dev(shape)[c0:L]
    counts = torch.tensor([c0, c1], dtype=torch.int32, device=DEV)
    p, v = _outputs(L + 8, hn.A)
    hn.forward_dev(x, counts.data_ptr(), 1, L, p, v, _stream())
    torch.cuda.synchronize()
    assert _untouched(p, v, np.arange(c0, L))
    pd, vd = _dense(hn, _pool_dev(shape)[c0:L])
    assert torch.equal(p[c0:L], pd) and torch.equal(v[c0:L], vd)
    _gate("c4", np.arange(c0, L), pd, vd, c1)
