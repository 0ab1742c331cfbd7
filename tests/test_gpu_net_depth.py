"""Residual towers of any depth on the HIP net kernels (k_net_forward_any / _w_any / _w2_any, caro_net_create_depth):
accuracy against torch at every tile class, a bit-level anchor to the depth-5 kernels (blocks whose folded weights are
zero change nothing), dispatch, pair launches of unequal depth, the search on top, and the command lines."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_NUMERICS_OPEN = []  # non-empty once this session has started the file
NUMERICS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "net_depth_numerics.txt")


def _net(shape, A, K, seed=0):
    """seeded weights, batch-norm running statistics and affine parameters randomised: the fold is exercised"""
    from caro_ai_amd.lib.model import Net
    torch.manual_seed(seed)
    net = Net(shape, A, n_residual=K)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.uniform_(-0.5, 0.5)
            m.running_var.uniform_(0.5, 2.0)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.uniform_(-0.3, 0.3)
    return net.eval()


def _boards(L, shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand((L,) + shape, generator=g) < 0.3).float()
    x[:, 1] *= (1 - x[:, 0])
    return x


def _zero_padded(net, extra):
    """`net` with `extra` more blocks whose folded weights and biases are exactly zero (batch-norm gamma = beta = 0,
    running mean 0): each contributes LeakyReLU(0) = +0 to h + block(h)"""
    from caro_ai_amd.lib.model import Net
    deep = Net(net.input_shape, net.actions_n, n_residual=net.n_residual + extra)
    sd = deep.state_dict()
    sd.update(net.state_dict())
    for i in range(net.n_residual + 1, net.n_residual + extra + 1):
        sd["conv_%d.1.weight" % i].zero_()
        sd["conv_%d.1.bias" % i].zero_()
        sd["conv_%d.1.running_mean" % i].zero_()
        sd["conv_%d.0.bias" % i].zero_()
    deep.load_state_dict(sd)
    return deep.eval()


def _shipped():
    from caro_ai_amd.lib.model import Net
    net = Net((2, 6, 7), 7)
    net.load_state_dict(torch.load(os.path.join(GOLDEN, "weights", "best_026_12000.dat"), map_location="cpu"))
    return net.eval()


def _recorded_boards(n):
    """planes of positions from the recorded connect-four fixtures (tests/golden/rules_c4.json.gz)"""
    from caro_ai_amd.lib.game.connect_four import ConnectFour
    game = ConnectFour()
    d = load_golden("rules_c4.json.gz")
    recs = d["recs"]
    states = [int(r["s"]) for r in recs[:n]]
    players = [int(r["p"]) for r in recs[:n]]
    assert len(states) == n
    return torch.as_tensor(np.asarray(game.states_to_training_batch(states, players)), dtype=torch.float32)


# row counts of tests/test_gpu_net.py: small tiles (4-way / 2-way K-split), a full tile, and (connect four, row form)
# a launch that overflows one round of full tiles
ROWS = {(6, 7): [1, 7, 29, 300, 1537], (3, 3): [1, 6, 300, 5500], (9, 9): [1, 5, 300], (15, 15): [1, 31, 257]}


@pytest.mark.parametrize("K", [1, 2, 3, 8, 12, 20])
@pytest.mark.parametrize("hw", [(6, 7), (3, 3), (9, 9), (15, 15)])
def test_any_depth_matches_torch_fp32(K, hw):
    """tests/test_gpu_net.py::test_hip_net_matches_torch_fp32's gates at depth K: the HIP outputs are no further from a
    float64 forward than max(4 x torch-fp32's own distance, 1e-6), the priors and (the same form, so that a deep net's
    value head is gated too) the values; the absolute gates |dP|, |dv| < 1e-4 are the project's numbers for five blocks
    and apply as they are for K <= 5 only.  The measured absolute errors of every case are
    printed, and collected in profiles/net_depth_numerics.txt (rewritten by the first case of a session) when
    CARO_WRITE_NUMERICS=1 -- the committed copy is such a run."""
    from caro_ai_amd.net_hip import HipNet
    H, W = hw
    shape, A = (2, H, W), (7 if hw == (6, 7) else H * W)
    net = _net(shape, A, K, seed=K)
    modes = ["f32", "f32w"] + (["f32w1", "f32w2"] if H >= 12 else [])
    lines = []
    for mode in modes:
        hn = HipNet(net, DEV, mode=mode)
        assert hn.L.caro_net_depth(hn.h) == K
        if mode == "f32w" and H >= 13:
            assert hn.mode == "f32w2"
        for L in ROWS[hw]:
            x = _boards(L, shape, L)
            with torch.no_grad():
                lg, vl = net(x)
                p_ref = torch.softmax(lg, dim=1)
                lg64, vl64 = net.double()(x.double())
                p64 = torch.softmax(lg64, dim=1)
            net.float()
            p, v = hn(x.to(DEV))
            torch.cuda.synchronize()
            p, v = p.cpu(), v.cpu()
            e_hip = (p.double() - p64).abs().max().item()
            e_ref = (p_ref.double() - p64).abs().max().item()
            ev_hip = (v.double() - vl64[:, 0]).abs().max().item()
            ev_ref = (vl[:, 0].double() - vl64[:, 0]).abs().max().item()
            dp, dv = (p - p_ref).abs().max().item(), (v - vl[:, 0]).abs().max().item()
            lines.append("K=%d board=%dx%d mode=%s rows=%d  |dP|=%.3e |dv|=%.3e  e_hip64=%.3e e_torch64=%.3e"
                         "  ev_hip64=%.3e ev_torch64=%.3e"
                         % (K, H, W, hn.mode if mode == "f32w" else mode, L, dp, dv, e_hip, e_ref, ev_hip, ev_ref))
            print(lines[-1])
            assert e_hip < max(4 * e_ref, 1e-6), (mode, L, e_hip, e_ref)
            assert ev_hip < max(4 * ev_ref, 1e-6), (mode, L, ev_hip, ev_ref)
            if K <= 5:
                assert dp < 1e-4 and dv < 1e-4, (mode, L, dp, dv)
            assert torch.allclose(p.sum(1), torch.ones(L), atol=1e-5)
        hn.close()
    if os.environ.get("CARO_WRITE_NUMERICS") == "1":
        with open(NUMERICS, "a" if _NUMERICS_OPEN else "w") as f:
            _NUMERICS_OPEN.append(1)
            f.write("\n".join(lines) + "\n")


@pytest.mark.parametrize("mode", ["f32", "f32w"])
def test_zero_blocks_behind_the_shipped_net_change_no_bit(mode):
    """the depth-8 twin of best_026_12000.dat (three blocks of zero weights appended) runs the run-time-depth kernels; its
    priors and values on 1 500 recorded-game boards are the shipped depth-5 net's bit for bit: full tiles, 2-way and
    4-way K-split tiles.  A differing bit would mean the run-time-depth instantiation does not do the per-layer
    arithmetic of the depth-5 one."""
    from caro_ai_amd.net_hip import HipNet
    five = _shipped()
    eight = _zero_padded(five, 3)
    x = _recorded_boards(1500).to(DEV)
    h5, h8 = HipNet(five, DEV, mode=mode), HipNet(eight, DEV, mode=mode)
    assert h5.L.caro_net_depth(h5.h) == 5 and h8.L.caro_net_depth(h8.h) == 8
    for rows in (1500, 700, 200, 6):  # full tiles, 2-way tiles, 4-way tiles, one small tile
        p5, v5 = h5(x[:rows])
        p8, v8 = h8(x[:rows])
        torch.cuda.synchronize()
        assert torch.equal(p5, p8) and torch.equal(v5, v8), (mode, rows)
    # bf16x3 is built for five blocks: a clear refusal, in Python and in the library
    from caro_ai_amd import _lib
    from caro_ai_amd.net_hip import pack_net_x3
    with pytest.raises(_lib.CaroError, match="5 residual blocks only"):
        HipNet(eight, DEV, mode="bf16x3")
    hf = HipNet(eight, DEV, mode="f32")
    wx = pack_net_x3(eight)
    assert hf.L.caro_net_enable_split_bf16(hf.h, wx.ctypes.data, wx.size) == -22
    assert b"5 residual blocks only" in hf.L.caro_last_error()
    # an image sized for another depth
    from caro_ai_amd.net_hip import pack_net_w
    w5 = pack_net_w(five)
    assert hf.L.caro_net_enable_winograd(hf.h, w5.ctypes.data, w5.size) == -22 and b"8 residual blocks" in hf.L.caro_last_error()
    for h in (h5, h8, hf):
        h.close()


def test_zero_blocks_on_15x15_in_the_2d_form_change_no_bit():
    from caro_ai_amd.net_hip import HipNet
    five = _net((2, 15, 15), 225, 5, seed=15)
    eight = _zero_padded(five, 3)
    h5, h8 = HipNet(five, DEV, mode="f32w"), HipNet(eight, DEV, mode="f32w")
    assert h5.mode == "f32w2" and h8.mode == "f32w2"
    x = _boards(300, (2, 15, 15), 9).to(DEV)
    p5, v5 = h5(x)
    p8, v8 = h8(x)
    torch.cuda.synchronize()
    assert torch.equal(p5, p8) and torch.equal(v5, v8)
    h5.close(); h8.close()


@pytest.mark.parametrize("mode", ["f32", "f32w"])
def test_depth_5_through_the_new_entry_point_is_caro_net_create(mode):
    """HipNet creates every net through caro_net_create_depth; a depth-5 net created through caro_net_create and run
    through the same launches gives the same bits (the same kernels)"""
    from caro_ai_amd import _lib
    from caro_ai_amd.net_hip import HipNet, pack_net, pack_net_w
    L = _lib.load()
    net = _shipped()
    hn = HipNet(net, DEV, mode=mode)
    packed = pack_net(net)
    old = C.c_void_p()
    _lib.check(L.caro_net_create(6, 7, 7, 0.01, packed.ctypes.data, packed.size, 0, C.byref(old)))
    assert L.caro_net_depth(old) == 5 == L.caro_net_depth(hn.h)
    if mode == "f32w":
        ww = pack_net_w(net)
        _lib.check(L.caro_net_enable_winograd(old, ww.ctypes.data, ww.size))
    for rows in (6, 300, 1500):
        x = _boards(rows, (2, 6, 7), rows).to(DEV)
        p, v = hn(x)
        counts = torch.tensor([rows, 0], dtype=torch.int32, device=DEV)
        p2 = torch.empty_like(p); v2 = torch.empty_like(v)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(L.caro_net_forward(old, x.data_ptr(), counts.data_ptr(), 0, rows, p2.data_ptr(), v2.data_ptr(), st))
        torch.cuda.synchronize()
        assert torch.equal(p, p2) and torch.equal(v, v2)
    L.caro_net_destroy(old)
    hn.close()


@pytest.mark.parametrize("mode", ["f32", "f32w"])
def test_pair_launch_of_unequal_depth_equals_two_single_launches(mode):
    """an arena between a 5-block and a 10-block net: one launch serving both gives the bits of one launch per net"""
    from caro_ai_amd import _lib
    from caro_ai_amd.net_hip import HipNet
    L = _lib.load()
    n0 = HipNet(_shipped(), DEV, mode=mode)
    n1 = HipNet(_net((2, 6, 7), 7, 10, seed=10), DEV, mode=mode)
    for a, b in ((n0, n1), (n1, n0)):
        for l0, l1 in [(13, 22), (0, 9), (6, 0), (12, 12), (1, 1)]:
            rows, cap = l0 + l1, 64
            x = torch.zeros((cap, 2, 6, 7), device=DEV)
            x[:rows] = _boards(rows, (2, 6, 7), rows + 1).to(DEV)
            counts = torch.tensor([l0, l1], dtype=torch.int32, device=DEV)
            pa = torch.full((cap, 7), -1.0, device=DEV); va = torch.full((cap,), -9.0, device=DEV)
            pb = torch.full((cap, 7), -1.0, device=DEV); vb = torch.full((cap,), -9.0, device=DEV)
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(L.caro_net_forward_pair(a.h, b.h, x.data_ptr(), counts.data_ptr(), cap, pa.data_ptr(),
                                               va.data_ptr(), st))
            a.forward_dev(x, counts.data_ptr(), 0, cap, pb, vb, st)
            b.forward_dev(x, counts.data_ptr(), 1, cap, pb, vb, st)
            torch.cuda.synchronize()
            assert torch.equal(pa, pb) and torch.equal(va, vb), (l0, l1)
            assert (pa[rows:] == -1).all()
    n0.close(); n1.close()


def test_pair_launch_of_unequal_depth_on_15x15_in_the_2d_form():
    """k_net_forward_w2_any + k_net_heads serving a 5-block and a 10-block net in one launch: the bits of one launch per net"""
    from caro_ai_amd import _lib
    from caro_ai_amd.net_hip import HipNet
    L = _lib.load()
    shape, A = (2, 15, 15), 225
    n0 = HipNet(_net(shape, A, 5, seed=1), DEV, mode="f32w")
    n1 = HipNet(_net(shape, A, 10, seed=2), DEV, mode="f32w")
    assert n0.mode == n1.mode == "f32w2"
    for a, b in ((n0, n1), (n1, n0)):
        for l0, l1 in [(40, 60), (0, 33), (7, 0)]:
            rows = l0 + l1
            x = _boards(rows, shape, rows).to(DEV)
            counts = torch.tensor([l0, l1], dtype=torch.int32, device=DEV)
            pa = torch.full((rows, A), -1.0, device=DEV); va = torch.full((rows,), -9.0, device=DEV)
            pb = torch.full((rows, A), -1.0, device=DEV); vb = torch.full((rows,), -9.0, device=DEV)
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(L.caro_net_forward_pair(a.h, b.h, x.data_ptr(), counts.data_ptr(), rows, pa.data_ptr(),
                                               va.data_ptr(), st))
            a.forward_dev(x, counts.data_ptr(), 0, rows, pb, vb, st)
            b.forward_dev(x, counts.data_ptr(), 1, rows, pb, vb, st)
            torch.cuda.synchronize()
            assert torch.equal(pa, pb) and torch.equal(va, vb), (l0, l1)
    n0.close(); n1.close()


@pytest.mark.parametrize("hw,A", [((6, 7), 7), ((15, 15), 225)])
def test_slot_launch_of_two_nets_of_unequal_depth(hw, A):
    """caro_net_forward_slots (the fused tree kernel's row form: game g's j-th leaf at row g * B + j, gpack = count |
    class << 8) with a 5-block and a 10-block net: every game's rows carry the bits of a single-net slot launch of its
    own net (connect four: 4-way tiles of one board; 15x15: one board per workgroup -- a row's arithmetic does not
    depend on its tile).  The slot forms against DENSE launches, at every tile class: tests/test_gpu_net_launch_forms.py."""
    from caro_ai_amd import _lib
    from caro_ai_amd.net_hip import HipNet
    L = _lib.load()
    shape = (2,) + hw
    n0 = HipNet(_net(shape, A, 5, seed=5), DEV)
    n1 = HipNet(_net(shape, A, 10, seed=6), DEV)
    G, B = 16, 8
    rng = np.random.default_rng(3)
    cnt = rng.integers(0, B + 1, G)
    cls = rng.integers(0, 2, G)
    x = _boards(G * B, shape, 77).to(DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch(a, b, classes):
        gpack = torch.tensor((cnt | (classes << 8)).astype(np.int32), device=DEV)
        counts = torch.tensor([int(cnt[classes == 0].sum()), int(cnt[classes == 1].sum())], dtype=torch.int32, device=DEV)
        p = torch.full((G * B, A), -1.0, device=DEV); v = torch.full((G * B,), -9.0, device=DEV)
        _lib.check(L.caro_net_forward_slots(a.h, b.h if b else None, x.data_ptr(), counts.data_ptr(), gpack.data_ptr(),
                                            G, B, p.data_ptr(), v.data_ptr(), st))
        torch.cuda.synchronize()
        return p.cpu().numpy().reshape(G, B, A), v.cpu().numpy().reshape(G, B)

    p2, v2 = launch(n0, n1, cls)
    pa, va = launch(n0, None, cls)        # net 0 alone: the class-0 games
    pb, vb = launch(n1, None, 1 - cls)    # net 1 alone, its games presented as class 0
    for g in range(G):
        ps, vs = (pa, va) if cls[g] == 0 else (pb, vb)
        assert np.array_equal(p2[g, :cnt[g]], ps[g, :cnt[g]]) and np.array_equal(v2[g, :cnt[g]], vs[g, :cnt[g]]), g
        assert (p2[g, cnt[g]:] == -1).all()
    n0.close(); n1.close()


def test_slot_list_launch_of_two_nets_of_unequal_depth_on_15x15():
    """caro_net_forward_slot_list (the multi-wave tree kernel's form: the dense order of each net's leaves GIVEN, here
    shuffled) with a 5-block and a 10-block net in the 2-D form, the one form that reads the list: every row carries
    the bits of the game-order slot launch of the same two nets.  The list against DENSE launches, and a wrong list where it
    is ignored: tests/test_gpu_net_launch_forms.py."""
    from caro_ai_amd import _lib
    from caro_ai_amd.net_hip import HipNet
    L = _lib.load()
    shape, A = (2, 15, 15), 225
    n0 = HipNet(_net(shape, A, 5, seed=5), DEV)
    n1 = HipNet(_net(shape, A, 10, seed=6), DEV)
    assert L.caro_net_uses_slot_list(n0.h) == 1 == L.caro_net_uses_slot_list(n1.h)
    G, B = 16, 8
    rng = np.random.default_rng(4)
    cnt = rng.integers(0, B + 1, G)
    cls = rng.integers(0, 2, G)
    x = _boards(G * B, shape, 78).to(DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    gpack = torch.tensor((cnt | (cls << 8)).astype(np.int32), device=DEV)
    counts = torch.tensor([int(cnt[cls == 0].sum()), int(cnt[cls == 1].sum())], dtype=torch.int32, device=DEV)
    slist = np.full((2, G * B), -1, np.int32)
    for c in (0, 1):
        rows = np.array([g * B + j for g in range(G) if cls[g] == c for j in range(cnt[g])], np.int32)
        slist[c, :len(rows)] = rng.permutation(rows)
    slist = torch.tensor(slist, device=DEV)
    for a, b in ((n0, n1), (n1, n0)):
        out = []
        for sl in (None, slist.data_ptr()):
            p = torch.full((G * B, A), -1.0, device=DEV); v = torch.full((G * B,), -9.0, device=DEV)
            _lib.check(L.caro_net_forward_slot_list(a.h, b.h, x.data_ptr(), counts.data_ptr(), gpack.data_ptr(), sl, G, B,
                                                    p.data_ptr(), v.data_ptr(), st))
            torch.cuda.synchronize()
            out.append((p.cpu(), v.cpu()))
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
        used = np.zeros(G * B, bool)
        used[[g * B + j for g in range(G) for j in range(cnt[g])]] = True
        assert (out[1][0][torch.tensor(used)] >= 0).all() and (out[1][0][torch.tensor(~used)] == -1).all()
    n0.close(); n1.close()


def test_arena_of_a_5_and_a_10_block_net_plays_to_the_end():
    """two stores, two nets of unequal depth in the engine's own pair launches (lib.utils.play_games, as play.py)"""
    from caro_ai_amd.lib import utils
    from caro_ai_amd.lib.game.connect_four import ConnectFour
    game = ConnectFour()
    five, ten = _shipped().to(DEV), _net((2, 6, 7), 7, 10, seed=3).to(DEV)
    res = utils.play_games(game, 8, None, five, ten, steps_before_tau_0=0, mcts_searches=4, mcts_batch_size=8,
                           concurrent=8, seed=1, uid_base=0, device=DEV, first_player_mode=2)
    assert len(res) == 8 and all(r in (-1, 0, 1) for r in res)


def _by_uid(tuples, games):
    out, off = {}, 0
    PI = np.concatenate([t["pi"] for t in tuples]); ST = np.concatenate([t["states"] for t in tuples])
    for uid, first, result, steps in games.tolist():
        n = steps + 1
        out[uid] = (first, result, steps, ST[off:off + n].tobytes(), PI[off:off + n].tobytes())
        off += n
    return out


@pytest.mark.parametrize("kind,G,S,B", [("c4", 64, 10, 8), ("mnk9", 32, 5, 8)])
def test_staggered_engine_plays_the_lock_step_games_with_a_depth_3_net(kind, G, S, B):
    """tests/test_gpu_stagger.py's property for the shipped net, with a seeded 3-block net: the net is a handle, the
    engine does not know its depth"""
    from caro_ai_amd.engine import SelfPlayEngine, staggered_geometry
    from caro_ai_amd.lib.game.connect_four import ConnectFour
    from caro_ai_amd.lib.game.tictactoe import TicTacToe
    game = ConnectFour() if kind == "c4" else TicTacToe(9, 5)
    net = _net(game.obs_shape, game.action_space, 3, seed=33).to(DEV)
    hw = game.obs_shape[1] * game.obs_shape[2]
    evict = S * B * hw + 64 > SelfPlayEngine.DEFAULT_CAP_LIMIT  # as lib.utils.play_games picks it
    assert staggered_geometry(game, B, evict)
    out = []
    for stagger in (False, True):
        eng = SelfPlayEngine(game, G, net1=net, max_batch=B, seed=17, device=DEV, searches_hint=S, stagger=stagger,
                             evict=evict)
        tuples, games = eng.play_until(S, B, n_finished=G)
        assert eng.counters()["overflows"] == 0
        eng.close()
        out.append(_by_uid(tuples, games))
    common = set(out[0]) & set(out[1])
    assert len(common) >= G * 3 // 4
    for uid in common:
        assert out[0][uid] == out[1][uid], uid


def test_fused_search_on_a_depth_8_net_carries_the_torch_searchs_visits():
    """MCTS.search_batch's fused path (HIP kernel) against the same search driven step-wise by the torch module on the CPU,
    from every ply of the recorded connect-four games, each root on a fresh tree: DESIGN section 2's tolerance -- the root
    visit vector is identical at >= 99 % of the roots, |d pi| <= 0.15 at the rest"""
    from caro_ai_amd.lib import mcts
    from caro_ai_amd.lib.game.connect_four import ConnectFour
    game = ConnectFour()
    d = load_golden("real_c4_x32.json.gz")
    roots = [(int(s), int(p)) for gm in d["games"] for s, p in zip(gm["states"], gm["players"])]
    roots = [(s, p) for s, p in roots if game.possible_moves(s)]
    assert len(roots) >= 200
    cpu_net = _net(game.obs_shape, game.action_space, 8, seed=8)
    gpu_net = _net(game.obs_shape, game.action_space, 8, seed=8).to(DEV)
    S, B = 6, 8
    same, worst = 0, 0.0
    for k, (s, p) in enumerate(roots):
        pis = []
        for net, dev in ((gpu_net, DEV), (cpu_net, "cpu")):
            np.random.seed(1000 + k)
            tree = mcts.MCTS(game, tree_device=DEV)
            tree.search_batch(S, B, s, p, net, device=dev)
            pis.append(np.asarray(tree.get_policy_value(s, tau=1)[0]))
        if np.array_equal(pis[0], pis[1]):
            same += 1
        worst = max(worst, float(np.abs(pis[0] - pis[1]).max()))
    print("fused vs step-wise torch search, depth 8: identical root visits at %d / %d roots, worst |d pi| %.3f"
          % (same, len(roots), worst))
    assert same / len(roots) >= 0.99 and worst <= 0.15


def test_command_lines_train_a_3_block_net_and_play_it(tmp_path, monkeypatch):
    """`train -g 0 --res-blocks 3` for two iterations writes best_*.dat; play.py and Session build the net from the
    checkpoint's own depth and play to the end; bf16x3 beside --res-blocks 3 exits with the documented error"""
    from caro_ai_amd import config as cfg
    from caro_ai_amd import play, train
    from caro_ai_amd.lib.game.connect_four import ConnectFour
    from caro_ai_amd.lib.model import state_dict_depth
    from caro_ai_amd.lib.play_session import Session
    monkeypatch.setattr(cfg, "MIN_REPLAY_TO_TRAIN", 300)
    monkeypatch.setattr(cfg, "EVALUATE_EVERY_STEP", 1)
    monkeypatch.setattr(cfg, "BEST_NET_WIN_RATIO", -1.0)  # always promote: a checkpoint per iteration
    monkeypatch.setattr(cfg, "EVALUATION_ROUNDS", 2)
    monkeypatch.setattr(cfg, "BATCH_SIZE", 32)
    monkeypatch.setattr(cfg, "TRAIN_ROUNDS", 2)
    train.release_engines()
    train.main(["-n", "d3", "-g", "0", "--cuda", "--res-blocks", "3", "--games", "32", "--iterations", "2",
                "--saves", str(tmp_path)])
    train.release_engines()
    files = sorted(os.listdir(tmp_path / "d3"))
    assert files and all(f.startswith("best_") and f.endswith(".dat") for f in files)
    last = str(tmp_path / "d3" / files[-1])
    assert state_dict_depth(torch.load(last, map_location="cpu")) == 3
    game = ConnectFour()
    assert play.load_checkpoint(game, last, DEV).n_residual == 3
    shipped = os.path.join(GOLDEN, "weights", "best_026_12000.dat")
    per_agent, per_pair = play.main(["-g", "0", "--cuda", last, shipped, "-r", "2"])  # a 3-block against the 5-block net
    assert sum(sum(v) for v in per_pair.values()) == 2 * 2
    monkeypatch.setattr(cfg, "BOT_MCTS_SEARCHES", 4)
    sess = Session(game, last, player_moves_first=False, device=DEV)
    assert sess.model.n_residual == 3
    rng = np.random.default_rng(0)
    for _ in range(42):
        if sess.move_bot() or sess.is_draw():
            break
        moves = game.possible_moves(sess.state)
        if sess.move_player(int(rng.choice(moves))) or sess.is_draw():
            break
    else:
        raise AssertionError("the game did not end")
    with pytest.raises(SystemExit, match="5 residual blocks only"):
        train.main(["-n", "d3x", "-g", "0", "--cuda", "--res-blocks", "3", "--net-mode", "bf16x3", "--iterations", "1",
                    "--saves", str(tmp_path)])
