"""Residual towers of any depth (`Net(..., n_residual=K)`, the `caro_net_*_depth` calls, `pack_net*`): everything that
can be said without a GPU -- checkpoint names, the torch forms, the packers as per-layer maps, the C-ABI's refusals.
The kernels themselves are tests/test_gpu_net_depth.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from caro_ai_amd import _lib
from caro_ai_amd.lib.model import FoldedNet, GemmNet, Net, _fold, state_dict_depth
from caro_ai_amd.net_hip import W2_PHASE_B, pack_net, pack_net_w, pack_net_w2, pack_net_x3
from tests.conftest import GOLDEN

SHIPPED = os.path.join(GOLDEN, "weights", "best_026_12000.dat")
C4 = ((2, 6, 7), 7)
DEPTHS = [1, 3, 5, 8, 20]


def _seeded(shape, A, K, seed=0):
    """a net whose batch-norm statistics and affine parameters are not the identity: the fold is exercised"""
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


def test_state_dict_names_follow_the_depth():
    shape, A = C4
    base = Net(shape, A).state_dict()
    five = Net(shape, A, n_residual=5).state_dict()
    assert len(base) == 62 and list(base) == list(five)
    assert all(base[k].shape == five[k].shape for k in base)
    Net(shape, A).load_state_dict(torch.load(SHIPPED, map_location="cpu"))  # the shipped checkpoint loads as before
    assert state_dict_depth(torch.load(SHIPPED, map_location="cpu")) == 5
    fixed = {k for k in base if not k.startswith("conv_") or k.split(".")[0] in ("conv_in", "conv_val", "conv_policy")}
    per_block = [k[len("conv_1"):] for k in base if k.startswith("conv_1.")]
    assert len(per_block) == 7
    for K in (1, 3, 8, 20):
        sd = Net(shape, A, n_residual=K).state_dict()
        want = fixed | {"conv_%d%s" % (i, s) for i in range(1, K + 1) for s in per_block}
        assert set(sd) == want and len(sd) == 62 - 35 + 7 * K
        assert state_dict_depth(sd) == K
        twin = Net.from_state_dict(sd, shape, A)
        assert twin.n_residual == K and len(twin.residual_blocks()) == K
    gap = {k: v for k, v in Net(shape, A, n_residual=3).state_dict().items() if not k.startswith("conv_2.")}
    with pytest.raises(ValueError, match="gap"):
        state_dict_depth(gap)
    with pytest.raises(ValueError):
        state_dict_depth({k: v for k, v in base.items() if k in fixed})
    with pytest.raises(ValueError):
        Net(shape, A, n_residual=0)


@pytest.mark.parametrize("K", [1, 3, 8])
def test_forward_is_a_loop_over_the_nets_own_blocks(K):
    shape, A = (2, 5, 5), 25
    net = _seeded(shape, A, K, seed=K).double()
    x = _boards(9, shape, K).double()
    with torch.no_grad():
        h = net.conv_in(x)
        for i in range(1, K + 1):
            h = h + getattr(net, "conv_%d" % i)(h)
        assert not hasattr(net, "conv_%d" % (K + 1))
        pol = net.policy(net.conv_policy(h).reshape(9, -1))
        val = net.value(net.conv_val(h).reshape(9, -1))
        got_p, got_v = net(x)
    assert torch.equal(got_p, pol) and torch.equal(got_v, val)


def test_folded_and_gemm_forms_of_a_depth_8_net():
    """tests/test_model.py's tolerances: |d logit| < 2e-4, |d v| < 2e-5 against Net.eval()"""
    shape, A = C4
    net = _seeded(shape, A, 8, seed=4)
    x = _boards(64, shape, 1)
    with torch.no_grad():
        lg, v = net(x)
        for form in (FoldedNet(net), GemmNet(net)):
            assert len(getattr(form, "ws", getattr(form, "wm", None))) in (8 + 3, 8 + 1)
            lf, vf = form(x)
            assert (lf - lg).abs().max().item() < 2e-4, type(form).__name__
            assert (vf - v).abs().max().item() < 2e-5, type(form).__name__


def _single_block_net(net, i):
    """a depth-1 net holding only block i of `net` (and its conv_in / heads)"""
    one = Net(net.input_shape, net.actions_n, n_residual=1)
    sd = {k: v for k, v in net.state_dict().items() if not (k.startswith("conv_") and k.split(".")[0][5:].isdigit())}
    sd.update({"conv_1" + k[len("conv_%d" % i):]: v for k, v in net.state_dict().items() if k.startswith("conv_%d." % i)})
    one.load_state_dict(sd)
    return one.eval()


@pytest.mark.parametrize("K", DEPTHS)
def test_packers_return_the_c_sizes_and_are_per_layer_maps(K):
    L = _lib.load()
    shape, A = C4
    if K == 5:  # today's images for the shipped weights, layer by layer
        net = Net(shape, A)
        net.load_state_dict(torch.load(SHIPPED, map_location="cpu"))
        net.eval()
        assert pack_net(net).size == L.caro_net_packed_size(6, 7, 7)
        assert pack_net_w2(net).size == L.caro_net_winograd2d_size() and pack_net_x3(net).size == L.caro_net_split_bf16_size()
    else:
        net = _seeded(shape, A, K, seed=K)
    flat, ww, w2, x3 = pack_net(net), pack_net_w(net), pack_net_w2(net), pack_net_x3(net)
    assert flat.size == L.caro_net_packed_size_depth(6, 7, 7, K)
    assert ww.size == L.caro_net_winograd_size_depth(K) == K * 12 * 4096
    assert w2.size == L.caro_net_winograd2d_size_depth(K) == K * 8 * 8192
    assert x3.size == L.caro_net_split_bf16_size_depth(K)
    head = 9 * 2 * 64 + 64
    wres = flat[head:head + K * 9 * 4096].reshape(K, -1)
    bres = flat[head + K * 9 * 4096:head + K * 9 * 4096 + K * 64].reshape(K, 64)
    tail = flat[head + K * 9 * 4096 + K * 64:]
    for i in sorted({1, (K + 1) // 2, K}):
        one = _single_block_net(net, i)
        f1 = pack_net(one)
        assert np.array_equal(f1[:head], flat[:head])
        assert np.array_equal(f1[head:head + 9 * 4096], wres[i - 1])
        assert np.array_equal(f1[head + 9 * 4096:head + 9 * 4096 + 64], bres[i - 1])
        assert np.array_equal(f1[head + 9 * 4096 + 64:], tail)
        assert np.array_equal(pack_net_w(one), ww.reshape(K, -1)[i - 1])
        assert np.array_equal(pack_net_w2(one), w2.reshape(K, -1)[i - 1])
        assert np.array_equal(pack_net_x3(one), x3.reshape(K, -1)[i - 1])


def test_new_symbols_and_refusals_without_a_gpu():
    L = _lib.load()
    for name in ("caro_net_create_depth", "caro_net_packed_size_depth", "caro_net_winograd_size_depth",
                 "caro_net_winograd2d_size_depth", "caro_net_split_bf16_size_depth", "caro_net_depth", "caro_net_max_depth"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.caro_version() >= 101
    top = L.caro_net_max_depth()
    assert 20 <= top <= 40
    assert L.caro_net_depth(None) == 0
    for K in (1, 5, 20, top):
        assert L.caro_net_packed_size_depth(6, 7, 7, K) == L.caro_net_packed_size(6, 7, 7) + (K - 5) * (9 * 4096 + 64)
    assert L.caro_net_winograd2d_size_depth(5) == L.caro_net_winograd2d_size()
    assert L.caro_net_split_bf16_size_depth(5) == L.caro_net_split_bf16_size()

    def refused(rc):
        assert rc == -22, rc  # CARO_E_INVAL
        msg = L.caro_last_error()
        assert msg and msg.strip()
        return msg.decode()

    for bad in (0, -1, top + 1, 1000):
        for fn in (L.caro_net_winograd_size_depth, L.caro_net_winograd2d_size_depth, L.caro_net_split_bf16_size_depth):
            assert "depth" in refused(fn(bad))
        assert "depth" in refused(L.caro_net_packed_size_depth(6, 7, 7, bad))
    # the create call: null, shape, depth, size -- and only then the device (caro_net_create's order)
    buf3 = np.zeros(L.caro_net_packed_size_depth(6, 7, 7, 3), np.float32)
    h = C.c_void_p()
    refused(L.caro_net_create_depth(6, 7, 7, 3, 0.01, None, buf3.size, 0, C.byref(h)))
    refused(L.caro_net_create_depth(6, 16, 7, 3, 0.01, buf3.ctypes.data, buf3.size, 0, C.byref(h)))
    for bad in (0, top + 1):
        assert "depth" in refused(L.caro_net_create_depth(6, 7, 7, bad, 0.01, buf3.ctypes.data, buf3.size, 0, C.byref(h)))
    # an image sized for another depth
    assert "3 residual blocks" in refused(L.caro_net_create_depth(6, 7, 7, 3, 0.01, buf3.ctypes.data,
                                                                 L.caro_net_packed_size(6, 7, 7), 0, C.byref(h)))
    refused(L.caro_net_create(6, 7, 7, 0.01, buf3.ctypes.data, buf3.size, 0, C.byref(h)))  # depth 5 wants its own size
    if not torch.cuda.is_available():
        rc = L.caro_net_create_depth(6, 7, 7, 3, 0.01, buf3.ctypes.data, buf3.size, 0, C.byref(h))
        assert rc == -19 and L.caro_last_error()  # CARO_E_NODEV, after every argument check


def test_runtime_depth_kernels_keep_the_registers_of_the_depth_5_ones():
    """the _any twins of the three float32 kernels: no spilled register, no scratch, at most 256 VGPRs (two waves per
    SIMD, as the depth-5 kernels) -- tests/test_cpu_product.py's rule for the hot kernels, applied to the new ones"""
    from tests.test_cpu_product import _code_object_metadata
    md = _code_object_metadata("caro_net.hip.o")
    twins = {n: k for n, k in md.items() if "_any" in n}
    assert len(twins) == 3, sorted(twins)
    for name, k in twins.items():
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0 and k[".vgpr_count"] <= 256, name
        assert k[".private_segment_fixed_size"] == 0, name
    for name in ("k_net_forwardE", "k_net_forward_wE", "k_net_forward_w2E", "k_net_forward_x3E"):
        assert sum(name in n for n in md) == 1, name  # the depth-5 kernels keep their names


def test_wino2d_image_of_a_depth_8_net_reproduces_its_layers():
    """tests/test_wino2d_cpu.py's numpy model of trunk_w2d's arithmetic (restated: that test is parametrised, not a
    function to call), on the packed image of a depth-8 net: every layer's two-phase fold gives torch's float64
    convolution, so the tower the kernel runs is Net.eval()'s"""
    n, K = 13, 8
    net = _seeded((2, n, n), n * n, K, seed=n)
    img = pack_net_w2(net).reshape(K, 8, 2, 4, 2, 64, 8).astype(np.float64)
    cols = {(0, 0): (1, 2, 1.0), (0, 1): (0, 2, -1.0), (1, 0): (2, 1, -1.0), (1, 1): (1, 3, -1.0)}  # (bh, phase) -> jA, jB, sg
    T = (n + 1) // 2
    x = torch.randn(1, 64, n, n, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    for layer in (0, 4, 7):
        w, _ = _fold(net.residual_blocks()[layer])
        ref = torch.nn.functional.conv2d(x, w.double(), padding=1)[0].numpy()
        U = np.zeros((2, 2, 4, 64, 64))  # [phase][bh][a][co][ci] read back from the image the way a lane finds it
        for ci in range(64):
            h, rem = divmod(ci, 32)
            G, j = divmod(rem, 4)
            cq, gi = divmod(G, 2)
            for sl in range(2):
                m = (gi ^ ((np.arange(64) >> 3) & 1)) == sl
                chunks = img[layer][[cq, 4 + cq]]  # [phase][bh][a][h][co][8]: chunk = phase * 4 + cq
                U[:, :, :, m, ci] = chunks[:, :, :, h][:, :, :, m, sl * 4 + j]
        xp = np.zeros((64, n + 3, n + 3))
        xp[:, 1:n + 1, 1:n + 1] = x[0].numpy()
        out = np.zeros((64, 2 * T, 2 * T))
        for ty in range(T):
            for tx in range(T):
                d = xp[:, 2 * ty:2 * ty + 4, 2 * tx:2 * tx + 4]
                Z = {}
                for (bh, phase), (jA, jB, sg) in cols.items():
                    c = d[:, :, jA] + sg * d[:, :, jB]
                    V = np.stack([c[:, 0] - c[:, 2], c[:, 1] + c[:, 2], c[:, 2] - c[:, 1], c[:, 1] - c[:, 3]])
                    M = np.einsum("aoi,ai->ao", U[phase, bh], V)
                    Z[(bh, phase)] = ((M[0] + M[1]) + M[2], (M[1] - M[2]) - M[3])
                for u_ in range(2):
                    out[:, 2 * ty + u_, 2 * tx] = (Z[(0, 1)][u_] + Z[(0, 0)][u_]) + Z[(1, 0)][u_]
                    out[:, 2 * ty + u_, 2 * tx + 1] = (Z[(0, 0)][u_] - Z[(1, 0)][u_]) - Z[(1, 1)][u_]
        err = np.abs(out[:, :n, :n] - ref).max()
        assert err < 5e-6 * max(1.0, np.abs(ref).max()), (layer, err)
    assert W2_PHASE_B == ((1, 2), (0, 3))


def test_train_cli_takes_the_depth_and_refuses_bf16x3_beside_it():
    from caro_ai_amd import train
    assert train.parse_args(["-n", "x", "-g", "0"]).res_blocks == 5
    assert train.parse_args(["-n", "x", "-g", "0", "--res-blocks", "12"]).res_blocks == 12
    with pytest.raises(SystemExit, match="5 residual blocks only"):
        train.main(["-n", "x", "-g", "0", "--res-blocks", "3", "--net-mode", "bf16x3"])
    with pytest.raises(SystemExit, match="--res-blocks must be in"):
        train.main(["-n", "x", "-g", "0", "--res-blocks", "0"])


def _depth_worker(rank, world, port, q):
    """two gloo ranks with 3-block nets of different seeds: the flat weight broadcast and the flat gradient bucket"""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from caro_ai_amd import parallel
    parallel.init(backend="gloo")
    torch.manual_seed(10 + rank)
    net = Net((2, 3, 3), 9, n_residual=3)
    parallel.broadcast_weights(net, src=0)
    sd = {k: v.numpy().copy() for k, v in net.state_dict().items()}
    x = _boards(4, (2, 3, 3), 50 + rank)
    pol, val = net(x)
    (pol.sum() + val.sum()).backward()
    own = [p.grad.numpy().copy() for p in net.parameters()]
    parallel.allreduce_grads(list(net.parameters()))
    q.put((rank, sd, own, [p.grad.numpy().copy() for p in net.parameters()]))
    dist.barrier()
    dist.destroy_process_group()


def test_weight_broadcast_ddp_bucket_and_netwrapper_at_depth_3():
    """`broadcast_weights`, `allreduce_grads` and `NetWrapper.sync` work on whatever state_dict they get: with a 3-block
    net every rank ends with rank 0's 48 tensors bit for bit, the reduced gradients are the sum of the ranks' own,
    and the frozen copy follows the trained net"""
    import socket
    import torch.multiprocessing as mp
    from caro_ai_amd.lib.model import NetWrapper
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_depth_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {r: rest for r, *rest in (q.get(timeout=120) for _ in range(2))}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    torch.manual_seed(10)
    want = Net((2, 3, 3), 9, n_residual=3).state_dict()
    assert len(want) == 62 - 35 + 7 * 3
    for r in range(2):
        assert list(res[r][0]) == list(want)
        for k in want:
            assert np.array_equal(res[r][0][k], want[k].numpy()), (r, k)
    for g0, g1, s0, s1 in zip(res[0][1], res[1][1], res[0][2], res[1][2]):
        assert np.array_equal(s0, s1) and np.array_equal(s0, g0 + g1)
    wrap = NetWrapper(_seeded((2, 3, 3), 9, 3, seed=1))
    assert wrap.target_model.n_residual == 3
    with torch.no_grad():
        for p in wrap.model.parameters():
            p.add_(1.0)
    wrap.sync()
    for a, b in zip(wrap.model.state_dict().values(), wrap.target_model.state_dict().values()):
        assert torch.equal(a, b)


def test_a_net_deeper_than_the_kernels_is_refused_with_the_librarys_text():
    from caro_ai_amd.net_hip import HipNet
    top = _lib.load().caro_net_max_depth()
    with pytest.raises(_lib.CaroError, match="unsupported net depth %d" % (top + 1)):
        HipNet(Net((2, 3, 3), 9, n_residual=top + 1), "cuda:0")
