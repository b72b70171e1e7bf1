"""The native single-scale SSIM criterion on the GPU (csrc/ssim_loss_kernels.hip, include/sstem_loss.h, loss/loss_ssim.py: SSIMLoss,
train_utils.SSIMMeanLoss, steps.IFNetStep(loss="ssim")) against ``ref64`` (tests/ssim_loss_ref64.py: the reference's formulation in
float64, on the GPU).

Bounds: |native - ref64| <= 4 D, D = the largest deviation of the REFERENCE's own fp32 run from float64 over the cases of
tests/golden/ssim_loss.npz for that quantity (value: absolute; gradient: max-norm relative to the gradient's max), read from the file.
The factor 4 and taking D over the cases are tests/test_ms_ssim_gpu.py's, for its reasons: another summation order and separable taps
are each a rounding pattern of the reference's own size, and one case's deviation is a single noisy sample."""
import os

import numpy as np
import pytest
import torch

import ssim_loss_ref64 as R
import sstem_native

pytestmark = pytest.mark.gpu

GUARD = 64              # floats either side of every buffer of a guarded call
SENTINEL = -777.25


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "ssim_loss.npz"))


@pytest.fixture(scope="module")
def bounds(golden):
    n = len(R.CASES)
    return {q: 4.0 * max(float(golden["c%d_dev_%s" % (i, q)]) for i in range(n)) for q in ("value", "grad")}


_pairs, _refs = {}, {}


def _pair(golden, i):
    if i not in _pairs:
        k = "c%d_" % i
        _pairs[i] = (torch.from_numpy(golden[k + "pred"]).cuda(), torch.from_numpy(golden[k + "target"]).cuda(), bool(golden[k + "size_average"]))
    return _pairs[i]


def _ref(golden, i):
    """ref64 of a case, computed once: value and the gradients with respect to both images (float64, on the GPU), grad_value = ones."""
    if i not in _refs:
        p, t, sa = _pair(golden, i)
        _refs[i] = R.ref64(p, t, sa, want_grad2=True)
    return _refs[i]


def _relmax(got, want):
    return float((got.double() - want).abs().max()) / float(want.abs().max())


class _Entries:
    """The three C-ABI entries on torch tensors; one zeroed-once workspace that is never cleared again."""

    def __init__(self, floats=1 << 16):
        self.lib = sstem_native.load_library()
        self.ws = torch.zeros(floats, dtype=torch.float32, device="cuda")

    def need(self, shape):
        return int(self.lib.sstem_ssim_loss_workspace_floats(*shape))

    def forward(self, a, b, per_sample, value=None, ws=None):
        ws = self.ws if ws is None else ws
        assert self.need(a.shape) <= ws.numel()
        if value is None:
            value = torch.empty((a.shape[0],) if per_sample else (), dtype=torch.float32, device="cuda")
        rc = self.lib.sstem_ssim_loss_forward_f32(a.data_ptr(), b.data_ptr(), *a.shape, int(per_sample), value.data_ptr(), ws.data_ptr(),
                                                  torch.cuda.current_stream().cuda_stream)
        sstem_native.check(rc, "sstem_ssim_loss_forward_f32")
        return value

    def backward(self, a, b, per_sample, grad_value=None, grad=None, ws=None):
        ws = self.ws if ws is None else ws
        if grad is None:
            grad = torch.empty_like(a)
        rc = self.lib.sstem_ssim_loss_backward_f32(a.data_ptr(), b.data_ptr(), *a.shape, int(per_sample),
                                                   grad_value.data_ptr() if grad_value is not None else None, grad.data_ptr(),
                                                   ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
        sstem_native.check(rc, "sstem_ssim_loss_backward_f32")
        return grad


@pytest.fixture(scope="module")
def entries():
    return _Entries()


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=lambda i: "c%d-%s" % (i, "x".join(map(str, R.CASES[i][0]))))
def test_value_and_every_gradient_element_against_ref64(golden, bounds, entries, i):
    pred, target, sa = _pair(golden, i)
    v64, g1_64, g2_64 = _ref(golden, i)
    value = entries.forward(pred, target, not sa)
    g1 = entries.backward(pred, target, not sa)
    g2 = entries.backward(target, pred, not sa)              # the img2 gradient: the same call with the two pointers exchanged
    torch.cuda.synchronize()
    dv = float((value.double() - v64).abs().max())
    d1, d2 = _relmax(g1, g1_64), _relmax(g2, g2_64)
    print("case %d %s: value %.3e (bound %.3e) grad img1 %.3e img2 %.3e (bound %.3e)" % (i, R.CASES[i][0], dv, bounds["value"], d1, d2, bounds["grad"]))
    assert value.shape == v64.shape and torch.isfinite(value).all() and torch.isfinite(g1).all() and torch.isfinite(g2).all()
    assert dv <= bounds["value"]
    assert d1 <= bounds["grad"] and d2 <= bounds["grad"]
    # the function is symmetric: the value with the images exchanged is within the same bound
    assert float((entries.forward(target, pred, not sa).double() - v64).abs().max()) <= bounds["value"]
    # the reference's own fp32 numbers are D away from ref64, so D + 4 D from the native ones
    k = "c%d_" % i
    assert float((value.double().cpu() - torch.as_tensor(golden[k + "value"]).double()).abs().max()) <= 1.25 * bounds["value"]
    assert _relmax(g1.cpu(), torch.from_numpy(golden[k + "grad"]).double()) <= 1.25 * bounds["grad"]


def test_grad_value_null_scalar_and_vector(golden, bounds, entries):
    # a scalar on a size_average case
    pred, target, sa = _pair(golden, 2)
    gv = torch.tensor(-0.375, device="cuda")
    _, g64 = R.ref64(pred, target, sa, grad_value=gv)
    assert _relmax(entries.backward(pred, target, not sa, gv), g64) <= bounds["grad"]
    assert torch.equal(entries.backward(pred, target, not sa, torch.ones((), device="cuda")), entries.backward(pred, target, not sa, None))
    # a [B] vector on the per-sample case; NULL there is a vector of ones
    pred, target, sa = _pair(golden, 5)
    assert not sa
    gv = torch.tensor([0.5, -2.0, 3.0], device="cuda")
    _, g64 = R.ref64(pred, target, sa, grad_value=gv)
    g = entries.backward(pred, target, True, gv)
    assert _relmax(g, g64) <= bounds["grad"]
    g_ones = entries.backward(pred, target, True, None)
    assert torch.equal(entries.backward(pred, target, True, torch.ones(3, device="cuda")), g_ones)
    for b in range(3):                                       # each sample's gradient scales with its own entry alone
        assert _relmax(g[b], float(gv[b]) * g_ones[b].double()) <= 1e-6
    # the same images under size_average: the per-sample gradients over B
    assert _relmax(entries.backward(pred, target, False, None), g_ones.double() / 3) <= 1e-6


def test_bits_repeat_on_a_dirty_workspace_inside_guard_bands(golden):
    """Three rounds over every case on ONE workspace that is zeroed once and never again (the partial sums of the larger shapes stay in
    it), every buffer between sentinel bands: identical bits each round, untouched bands, clean counter."""
    lib = sstem_native.load_library()
    need = max(int(lib.sstem_ssim_loss_workspace_floats(*shape)) for shape, _ in R.CASES)
    e = _Entries(floats=16)                                  # only its call wrappers are used here
    ws_buf = torch.full((need + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    ws = ws_buf[GUARD:GUARD + need]
    ws.zero_()                                               # once
    first = {}
    for rep in range(3):
        for i in (4, 0, 3, 5, 6, 1, 2):                      # large before small: the small ones find stale partial sums
            pred, target, sa = _pair(golden, i)
            B = pred.shape[0]
            nv = 1 if sa else B
            vbuf = torch.full((nv + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
            gbuf = torch.full((pred.numel() + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
            value = vbuf[GUARD:GUARD + nv].view(() if sa else (B,))
            grad = gbuf[GUARD:GUARD + pred.numel()].view(pred.shape)
            e.forward(pred, target, not sa, value=value, ws=ws)
            e.backward(pred, target, not sa, None, grad=grad, ws=ws)
            torch.cuda.synchronize()
            for buf, n in ((vbuf, nv), (gbuf, pred.numel()), (ws_buf, need)):
                assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())
            assert int(ws[:1].view(torch.int32)) == 0            # the launch counter is left clean
            if rep == 0:
                first[i] = (value.clone(), grad.clone())
            else:
                assert torch.equal(value, first[i][0]) and torch.equal(grad, first[i][1])
    assert bool((ws[16:] != 0).any())                        # dirty: nobody cleared the partial sums


def test_graph_capture_replays_equal_eager(golden):
    import train_utils
    pred, target, _ = _pair(golden, 3)
    crit = train_utils.SSIMMeanLoss(pred.device)
    v_eager, g_eager = crit(pred, target)                    # also creates the workspace, outside the capture
    v_eager, g_eager = v_eager.clone(), g_eager.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        v, g = crit(pred, target)
    v.zero_(); g.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(v, v_eager) and torch.equal(g, g_eager)


def test_module_under_autograd_against_the_torch_formulation(golden, bounds):
    """SSIMLoss (native launches behind an autograd.Function) against ssim_loss_torch under autograd, both images requiring a gradient:
    the torch formulation in fp32 is the reference's own arithmetic, D from ref64, so D + 4 D from the native numbers."""
    from loss.loss_ssim import SSIMLoss, ssim, ssim_loss_torch
    for i in (0, 3, 5):
        pred, target, sa = _pair(golden, i)
        a, b = pred.clone().requires_grad_(True), target.clone().requires_grad_(True)
        out = SSIMLoss(size_average=sa)(a, b)
        out.sum().backward()
        a2, b2 = pred.clone().requires_grad_(True), target.clone().requires_grad_(True)
        want = ssim_loss_torch(a2, b2, sa)
        want.sum().backward()
        assert out.shape == want.shape
        assert float((out.detach() - want.detach()).abs().max()) <= 1.25 * bounds["value"]
        assert _relmax(a.grad, a2.grad.double()) <= 1.25 * bounds["grad"] and _relmax(b.grad, b2.grad.double()) <= 1.25 * bounds["grad"]
        # ssim() is the similarity: 1 - the loss (one fp32 subtraction away)
        assert float((ssim(pred, target, size_average=sa) - (1 - out.detach())).abs().max()) <= 1.2e-7
        # img1 alone: the same gradient, nothing computed for img2
        a3 = pred.clone().requires_grad_(True)
        SSIMLoss(size_average=sa)(a3, target).sum().backward()
        assert torch.equal(a3.grad, a.grad)
    with pytest.raises(TypeError):
        SSIMLoss()(pred.half(), target.half())
    # through autograd arithmetic on the value: a [B] grad_value reaches the launch
    pred, target, _ = _pair(golden, 5)
    wts = torch.tensor([0.5, -2.0, 3.0], device="cuda")
    a = pred.clone().requires_grad_(True)
    (SSIMLoss(size_average=False)(a, target) * wts).sum().backward()
    _, g64 = R.ref64(pred, target, False, grad_value=wts)
    assert _relmax(a.grad, g64) <= bounds["grad"]


def test_calling_conventions_agree(golden):
    """``pred.backward(grad)`` from SSIMMeanLoss against ``SSIMLoss()(pred, target).backward()``: the same launches, the same bits."""
    import train_utils
    from loss.loss_ssim import SSIMLoss
    pred, target, _ = _pair(golden, 3)
    a = pred.clone().requires_grad_(True)
    v = SSIMLoss()(a, target)
    v.backward()
    loss, grad = train_utils.SSIMMeanLoss(pred.device)(pred, target)
    assert torch.equal(loss, v.detach()) and torch.equal(grad, a.grad)


def test_ifnet_step_ssim_native_against_torch(bounds, monkeypatch):
    """steps.IFNetStep(loss="ssim"): native against SSTEM_NATIVE_SSIM=0 after one forward_backward (same seed: same weights and batch),
    by the rule tests/test_ms_ssim_gpu.py applies to its FusionStep pair: the losses within the value bound, the flat gradients within
    the gradient bound of their max."""
    import steps
    import train_utils
    dev = torch.device("cuda")
    native = steps.IFNetStep(dev, global_batch=1, size=64, loss="ssim")
    assert isinstance(native.criterion, train_utils.SSIMMeanLoss) and native.loss_name == "ssim"
    native.forward_backward()
    torch.cuda.synchronize()
    g_native, v_native = native.buckets[0].flat.clone(), float(native.loss)
    assert np.isfinite(v_native) and 0.0 < v_native < 2.0

    monkeypatch.setattr(steps, "_NATIVE_SSIM", False)        # what SSTEM_NATIVE_SSIM=0 sets at import
    plain = steps.IFNetStep(dev, global_batch=1, size=64, loss="ssim")
    monkeypatch.undo()
    from loss.loss_ssim import ssim_loss_torch
    assert plain.criterion is ssim_loss_torch
    assert torch.equal(plain.x, native.x) and torch.equal(plain.target, native.target)
    plain.forward_backward()
    torch.cuda.synchronize()
    d = _relmax(g_native, plain.buckets[0].flat.double())
    print("ifnet step: loss native %.7f torch %.7f, flat gradient differs by %.3e of its max (bound %.3e)"
          % (v_native, float(plain.loss.detach()), d, bounds["grad"]))
    assert abs(v_native - float(plain.loss.detach())) <= bounds["value"]
    assert d <= bounds["grad"]


def test_ifnet_step_criteria():
    """The default is still L1 through the shared body; "l2" selects the native L2 criterion and a step moves the weights."""
    import steps
    import train_utils
    dev = torch.device("cuda")
    st = steps.IFNetStep(dev, global_batch=1, size=64)
    assert st.loss_name == "l1" and st.criterion is st._l1 and st._loss_backward.__func__ is steps._TrainStep._loss_backward
    l2 = steps.IFNetStep(dev, global_batch=1, size=64, loss="l2")
    assert isinstance(l2.criterion, train_utils.L2MeanLoss)
    before = l2.flat.flat.clone()
    l2.step()
    torch.cuda.synchronize()
    assert torch.isfinite(l2.loss) and float(l2.loss) > 0 and not torch.equal(l2.flat.flat, before)
