"""sstem_warp_bilinear_backward_f32 (csrc/warp_kernels.hip) and utils.image_warp_torch.DifferentiableSpatialTransformation on the
GPU, every element against tests/warp_grad_ref64.py.

Bounds (u = 2^-24; S, k, A per element from ref64):
    grad_flow    n u S, n = C + 4: the kernel forms  gx += g * (wy*(ic - ia) + uy*(id - ib))  -- sub, mul, add, mul by g on the path of
                 any tap, and C - 1 adds of the channel sum (the first add is to zero); a contraction to fma only removes roundings.
    grad_image   (k + 2) u A + k 2^-126: each contribution w*g takes two roundings (w = wx*wy, then times g), then k - 1 adds in any
                 order; the absolute term allows for an adder that flushes a subnormal partial sum (not measured either way).
    with accumulate_image on a pre-filled buffer p the same count over one more summand: (k + 2) u (A + |p|) + (k + 1) 2^-126.
Where the contract gives zero (S = 0, or no in-plane contribution) the bounds are zero: exact zeros must be stored, over sentinels.

Every call here runs with each buffer between sentinel bands, at an odd element offset from the allocation."""
import os

import numpy as np
import pytest
import torch

import sstem_native
import warp_grad_ref64 as R

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -777.25
TINY = 2.0 ** -126
FIXTURE = ("rand", "knots", "zero", "sides", "p1x1", "c1", "many")
SHAPES = ("s2x3x7x13", "s1x1x1x1", "many33x65", "wrap840")
MODES = ("both", "flow", "image")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "warp_grad.npz"))


_inputs, _refs = {}, {}


def _case(gold, name):
    """(image, flow, g) float32 numpy of a fixture case or of a named shape; made once."""
    if name in _inputs:
        return _inputs[name]
    if name in FIXTURE:
        v = (gold[name + "_img"], gold[name + "_flow"], gold[name + "_g"])
    else:
        rng = np.random.default_rng(11 + SHAPES.index(name))
        shape = {"s2x3x7x13": (2, 3, 7, 13), "s1x1x1x1": (1, 1, 1, 1), "many33x65": (1, 2, 33, 65), "wrap840": (3, 1, 840, 840)}[name]
        B, C, H, W = shape
        if name == "many33x65":
            flow = R.many_to_one_flow(B, H, W, 16.25, 40.5)           # 2145 contributions on each of four addresses per channel
        elif name == "s1x1x1x1":
            flow = np.array([[[[-0.25]], [[0.5]]]], np.float32)
        else:
            flow = rng.uniform(-4, 4, (B, 2, H, W)).astype(np.float32)
        v = (rng.random(shape, dtype=np.float32), flow, rng.standard_normal(shape).astype(np.float32))
    _inputs[name] = v
    return v


def _ref(gold, name):
    if name not in _refs:
        _refs[name] = R.ref64(*_case(gold, name))
    return _refs[name]


class Guarded:
    """A float32 buffer of ``shape`` between two sentinel bands, starting an odd number of elements into its allocation."""

    def __init__(self, shape, fill=None):
        n = int(np.prod(shape))
        self.n = n
        self.buf = torch.full((n + 2 * GUARD + 1,), SENTINEL, dtype=torch.float32, device="cuda")
        self.t = self.buf[GUARD + 1:GUARD + 1 + n].view(shape)
        assert (self.t.data_ptr() // 4) % 2 == 1 or n == 0
        if fill is not None:
            self.t.copy_(torch.as_tensor(fill))

    def intact(self):
        return bool((self.buf[:GUARD + 1] == SENTINEL).all()) and bool((self.buf[GUARD + 1 + self.n:] == SENTINEL).all())


def _entry(img, flow, g, gf, gi, accumulate=0):
    B, C, H, W = g.shape
    lib = sstem_native.load_library()
    rc = lib.sstem_warp_bilinear_backward_f32(img.data_ptr() if img is not None else None, flow.data_ptr(), g.data_ptr(),
                                              gf.data_ptr() if gf is not None else None, gi.data_ptr() if gi is not None else None,
                                              accumulate, B, C, H, W, torch.cuda.current_stream().cuda_stream)
    sstem_native.check(rc, "sstem_warp_bilinear_backward_f32")


def _run(case, mode="both", prefill=None):
    """One guarded call -> (grad_flow or None, grad_image or None) as float64 numpy; outputs start as sentinels (dirty)."""
    img, flow, g = case
    bufs = [Guarded(img.shape, img), Guarded(flow.shape, flow), Guarded(g.shape, g)]
    gf = Guarded(flow.shape) if mode in ("both", "flow") else None
    gi = Guarded(img.shape) if mode in ("both", "image") else None
    if gi is not None:
        gi.t.fill_(SENTINEL)
        if prefill is not None:
            gi.t.copy_(torch.as_tensor(prefill))
    if gf is not None:
        gf.t.fill_(SENTINEL)
    _entry(bufs[0].t if mode != "image" else None, bufs[1].t, bufs[2].t, gf.t if gf else None, gi.t if gi else None,
           accumulate=int(prefill is not None))
    torch.cuda.synchronize()
    for b in bufs + [x for x in (gf, gi) if x is not None]:
        assert b.intact(), "a guard band was written"
    for b, src in zip(bufs, case):
        assert np.array_equal(b.t.cpu().numpy(), src), "an input was written"
    return (gf.t.cpu().numpy().astype(np.float64) if gf else None, gi.t.cpu().numpy().astype(np.float64) if gi else None,
            gf.t.clone() if gf else None)


def _check_flow(name, got, r, C):
    bound = R.flow_bound(r, C + 4)
    err = np.abs(got - r["grad_flow"])
    print("%s: grad_flow worst error / bound %.3f (max |error| %.2e)" % (name, float((err / np.maximum(bound, 1e-300)).max()), err.max()))
    assert np.isfinite(got).all() and (err <= bound).all()
    assert not got[r["S"] == 0].any()                                   # exact zeros over the sentinels


def _check_image(name, got, r, prefill=None):
    if prefill is None:
        bound, want = R.image_bound(r, 2, TINY), r["grad_image"]
    else:
        p = prefill.astype(np.float64)
        bound, want = (r["k"] + 2) * R.U * (r["A"] + np.abs(p)) + (r["k"] + 1) * TINY, r["grad_image"] + p
    err = np.abs(got - want)
    print("%s: grad_image worst error / bound %.3f (max |error| %.2e, max k %d)" % (
        name, float((err / np.maximum(bound, 1e-300)).max()), err.max(), int(r["k"].max())))
    assert np.isfinite(got).all() and (err <= bound).all()
    if prefill is None:
        assert not got[r["k"] == 0].any()                               # cleared by the entry, over the sentinels
    else:
        assert np.array_equal(got[r["k"] == 0], p[r["k"] == 0])         # untouched where nothing lands


@pytest.mark.parametrize("name", FIXTURE + SHAPES)
def test_every_element_against_the_restatement(gold, name):
    case, r = _case(gold, name), _ref(gold, name)
    C = case[0].shape[1]
    gf_both, gi_both, bits_both = _run(case, "both")
    _check_flow(name, gf_both, r, C)
    _check_image(name, gi_both, r)
    gf_alone, none, bits_alone = _run(case, "flow")
    assert none is None and torch.equal(bits_both, bits_alone)          # bit-identical from run to run, whatever else is asked for
    _, gi_alone, _ = _run(case, "image")                                # image pointer NULL: the image gradient does not read it
    _check_image(name + " (alone)", gi_alone, r)
    if name in FIXTURE:                                                 # the reference's own fp32 autograd: its bound plus ours
        assert (np.abs(gf_both - gold[name + "_grad_flow"]) <= R.flow_bound(r, 2 * C + 12)).all()
        assert (np.abs(gi_both - gold[name + "_grad_img"]) <= R.image_bound(r, 2, TINY) + R.image_bound(r, 4)).all()
    if name == "wrap840":
        B, _, H, W = case[0].shape
        assert B * H * W > 256 * 32 * 256 and 2 * H * W < 256 * 32 * 256 < 3 * H * W     # the grid-stride loop wraps, into the last sample


def test_accumulate_adds_to_a_prefilled_buffer(gold):
    for name in ("rand", "sides", "many33x65"):
        case, r = _case(gold, name), _ref(gold, name)
        prefill = np.random.default_rng(5).standard_normal(case[0].shape).astype(np.float32)
        for mode in ("both", "image"):
            _, gi, _ = _run(case, mode, prefill=prefill)
            _check_image("%s accumulate (%s)" % (name, mode), gi, r, prefill)


@pytest.mark.parametrize("amp", ["3W", "1e30"])
def test_flows_far_outside_the_plane_give_exact_zeros(amp):
    rng = np.random.default_rng(3)
    B, C, H, W = 2, 3, 7, 13
    img, g = rng.random((B, C, H, W), dtype=np.float32), rng.standard_normal((B, C, H, W)).astype(np.float32)
    a = 3.0 * W if amp == "3W" else 1e30
    sign = rng.choice([-1.0, 1.0], (B, 2, H, W))
    flow = (sign * a).astype(np.float32)
    flow[:, 1] *= np.float32(H / W) if amp == "3W" else np.float32(1)      # 3 H in y: outside on that axis too
    flow[0, 1, :, :4] = 0.0                                                 # outside in x alone
    flow[1, 0, :, 4:8] = 0.5                                                # outside in y alone
    for mode in MODES:
        gf, gi, _ = _run((img, flow, g), mode)
        assert gf is None or not gf.any()
        assert gi is None or not gi.any()
    prefill = rng.standard_normal((B, C, H, W)).astype(np.float32)
    _, gi, _ = _run((img, flow, g), "image", prefill=prefill)
    assert np.array_equal(gi, prefill.astype(np.float64))


def test_graph_replay(gold):
    for name in ("rand", "many33x65"):
        case, r = _case(gold, name), _ref(gold, name)
        img, flow, g = (Guarded(a.shape, a) for a in case)
        gf, gi = Guarded(flow.t.shape), Guarded(img.t.shape)
        _entry(img.t, flow.t, g.t, gf.t, gi.t)
        torch.cuda.synchronize()
        eager = gf.t.clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _entry(img.t, flow.t, g.t, gf.t, gi.t)
        for _ in range(2):                                              # the clear is part of the capture: nothing doubles
            gf.t.fill_(SENTINEL)
            graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gf.t, eager)                                 # eager and replay: the same bits
        _check_image(name + " replayed", gi.t.cpu().numpy().astype(np.float64), r)
        assert all(b.intact() for b in (img, flow, g, gf, gi))


def test_adjoint_with_the_forward_kernel(gold):
    """<warp(image), g> = <image, grad_image(g)>: ties the new taps to the existing forward kernel.  Both sums in float64 from the
    kernels' fp32 outputs; the difference is inside the sum of the per-element bounds of the two sides (forward: wx*wy, times I, three
    adds = 5 roundings relative to sum |w| |I|)."""
    lib = sstem_native.load_library()
    for name in ("rand", "sides", "s2x3x7x13", "many33x65"):
        case, r = _case(gold, name), _ref(gold, name)
        img, flow, g = (torch.from_numpy(a).cuda() for a in case)
        out = torch.empty_like(img)
        sstem_native.check(lib.sstem_warp_bilinear_f32(img.data_ptr(), flow.data_ptr(), out.data_ptr(), *img.shape,
                                                       torch.cuda.current_stream().cuda_stream), "sstem_warp_bilinear_f32")
        _, gi, _ = _run(case, "image")
        lhs = float((out.cpu().numpy().astype(np.float64) * case[2]).sum())
        rhs = float((case[0].astype(np.float64) * gi).sum())
        bound = float((np.abs(case[2]) * 5 * R.U * r["out_abs"]).sum() + (np.abs(case[0]) * R.image_bound(r, 2, TINY)).sum())
        print("%s: <out, g> = %.9g, <image, grad_image> = %.9g, difference %.2e (bound %.2e)" % (name, lhs, rhs, abs(lhs - rhs), bound))
        assert abs(lhs - rhs) <= bound


# ---- the module --------------------------------------------------------------------------------------------------------------------
def _forward_bits(img, flow):
    lib = sstem_native.load_library()
    out = torch.empty_like(img)
    sstem_native.check(lib.sstem_warp_bilinear_f32(img.data_ptr(), flow.data_ptr(), out.data_ptr(), *img.shape,
                                                   torch.cuda.current_stream().cuda_stream), "sstem_warp_bilinear_f32")
    return out


def test_module_default_is_todays_call(gold):
    from utils.image_warp_torch import DifferentiableSpatialTransformation, SpatialTransformation
    img, flow, _ = (torch.from_numpy(a).cuda() for a in _case(gold, "rand"))
    warp = SpatialTransformation(use_gpu=True)
    out = warp(img.clone().requires_grad_(True), flow.permute(0, 2, 3, 1).clone().requires_grad_(True))
    assert out.grad_fn is None and not out.requires_grad
    assert torch.equal(out, _forward_bits(img, flow))
    # differentiable, but nothing requires a gradient (or autograd is off): no node, the forward's bits
    dwarp = DifferentiableSpatialTransformation(use_gpu=True)
    assert isinstance(dwarp, SpatialTransformation) and dwarp.use_gpu is True
    out = dwarp(img, flow.permute(0, 2, 3, 1))
    assert out.grad_fn is None and torch.equal(out, _forward_bits(img, flow))
    with torch.no_grad():
        out = dwarp(img.clone().requires_grad_(True), flow.permute(0, 2, 3, 1))
    assert out.grad_fn is None
    with pytest.raises(NotImplementedError):
        dwarp(torch.zeros(1, 1, 2, 2, requires_grad=True), torch.zeros(1, 2, 2, 2))


def test_module_differentiable_gradients_are_the_entrys(gold):
    from utils.image_warp_torch import DifferentiableSpatialTransformation
    case, r = _case(gold, "rand"), _ref(gold, "rand")
    img, flow, g = (torch.from_numpy(a).cuda() for a in case)
    gf_entry, gi_entry = torch.empty_like(flow), torch.empty_like(img)
    _entry(img, flow, g, gf_entry, gi_entry)
    warp = DifferentiableSpatialTransformation(use_gpu=True)
    a = img.clone().requires_grad_(True)
    f = flow.clone().requires_grad_(True)                               # [B,2,H,W] leaf; the module sees a permuted, non-contiguous view
    dm = f.permute(0, 2, 3, 1)
    assert not dm.is_contiguous()
    out = warp(a, dm)
    assert out.grad_fn is not None and torch.equal(out.detach(), _forward_bits(img, flow))
    out.backward(g)
    assert torch.equal(f.grad, gf_entry)                                # no atomics: the entry's bits
    _check_image("module", a.grad.cpu().numpy().astype(np.float64), r)  # atomics: inside the entry's bound
    # a leaf in the caller's [B,H,W,2] layout, contiguous and not
    for leaf in (flow.permute(0, 2, 3, 1).contiguous(), torch.empty_like(flow).copy_(flow).permute(0, 2, 3, 1)):
        leaf = leaf.detach().requires_grad_(True)
        warp(img, leaf).backward(g)
        assert leaf.grad.shape == (2, 9, 13, 2) and torch.equal(leaf.grad, gf_entry.permute(0, 2, 3, 1))


class _Spy:
    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)

        def wrapper(*args):
            self.calls.append((name, args))
            return fn(*args)
        return wrapper


def test_module_computes_only_what_is_asked_for_in_one_call(gold, monkeypatch):
    import utils.image_warp_torch as M
    img, flow, g = (torch.from_numpy(a).cuda() for a in _case(gold, "rand"))
    spy = _Spy(sstem_native.load_library())
    monkeypatch.setattr(M.sstem_native, "load_library", lambda: spy)
    warp = M.DifferentiableSpatialTransformation(use_gpu=True)
    for need_img, need_flow in ((False, True), (True, False), (True, True)):
        a = img.clone().requires_grad_(need_img)
        f = flow.permute(0, 2, 3, 1).contiguous().requires_grad_(need_flow)
        spy.calls.clear()
        warp(a, f).backward(g)
        back = [args for name, args in spy.calls if name == "sstem_warp_bilinear_backward_f32"]
        assert len(back) == 1
        image_ptr, _, _, gf_ptr, gi_ptr, accumulate = back[0][:6]
        assert (gf_ptr is not None) == need_flow and (gi_ptr is not None) == need_img and accumulate == 0
        assert (image_ptr is not None) == need_flow
        assert (a.grad is not None) == need_img and (f.grad is not None) == need_flow


def test_module_refuses_a_second_differentiation(gold):
    from utils.image_warp_torch import DifferentiableSpatialTransformation
    img, flow, g = (torch.from_numpy(a).cuda() for a in _case(gold, "c1"))
    f = flow.permute(0, 2, 3, 1).contiguous().requires_grad_(True)
    out = DifferentiableSpatialTransformation(use_gpu=True)(img, f)
    first, = torch.autograd.grad(out, f, g, create_graph=True)
    with pytest.raises(RuntimeError):
        first.sum().backward()
