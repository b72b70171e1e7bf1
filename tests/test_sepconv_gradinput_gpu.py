"""The sepconv input gradient on the GPU: both kernels (DIRECT = one lane per element, MFMA = the 64 x 64 gather tile) at every element
against the float64 reference of tests/sepconv_gradinput_ref64.py, against each other bit for bit, inside guard bands, on inputs whose
answer is exact, through the bf16 and any-filter-length entries, and through autograd under the opt-in switch.

Bound: |got - ref| <= n * 2^-24 * S at every element, n = N_GRADINPUT = 2610 (1 multiply + 2601 fmaf on the path of the first term of
the kernels' one chain; derived in sepconv_gradinput_ref64, never tuned).  The tile is 64 x 64 with a 50-wide reach, so the shapes are
the ones of the issue: padded planes of whole tiles, one past, two images, C = 1 / 2, widths 3 and 1 (mod 4), interior tiles next to
edge tiles, and channel chunks (C = 4, 6).  Run with -s for the WORST lines.
"""

import pytest
import torch
import torch.nn.functional as F

import libs.sepconv as sepconv_pkg
import libs.sepconv._ext.cunnex as cunnex
import sstem_native
from libs.sepconv.SeparableConvolution import SeparableConvolution, sepconv_gray
from model.sepconv import FunctionSepconv
from sepconv_cases import make_case
from sepconv_gradinput_ref64 import N_GRADINPUT, grad_input_ref64
from sepconv_ref64 import assert_within_rounding

pytestmark = pytest.mark.gpu
DIRECT, MFMA = cunnex.ALGO_DIRECT, cunnex.ALGO_MFMA
ALGOS = [(DIRECT, "direct"), (MFMA, "tiled")]
KINDS = ["randn", "softmax"]
SHAPES = [
    (1, 3, 1, 1),        # gI is the 51 x 51 outer product
    (1, 3, 14, 78),      # padded plane 64 x 128: whole tiles only
    (1, 3, 15, 79),      # one row and one column past whole tiles
    (2, 3, 37, 70),      # the second image's base offsets
    (1, 1, 64, 67),      # C = 1; width 3 (mod 4)
    (1, 2, 40, 129),     # C = 2; width 1 (mod 4)
    (1, 3, 130, 200),    # interior tiles whose whole reach lies inside the image, next to edge tiles
    (1, 4, 20, 70),      # channel chunks 3 + 1
    (1, 6, 20, 70),      # channel chunks 3 + 3
]
WORST = {}
_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    _CASES.clear()
    torch.cuda.empty_cache()
    for family in sorted(WORST):
        print("\nWORST err / (2^-24 S)  %-40s %8.2f" % (family, WORST[family]))


@pytest.fixture(autouse=True)
def _switch_off_and_auto():
    sepconv_pkg.set_input_gradient(False)
    cunnex.set_algorithm(cunnex.ALGO_AUTO)
    yield
    sepconv_pkg.set_input_gradient(False)
    cunnex.set_algorithm(cunnex.ALGO_AUTO)


def _case(shape, kind):
    """(g, ver, hor, ref, S) on the GPU; the float64 reference is computed once per (shape, kind) and never modified."""
    key = (shape, kind)
    if key not in _CASES:
        B, C, H, W = shape
        _, ver, hor, g = make_case(4000 + 13 * B + 7 * C + H + W, B, C, H, W, kind)
        g, ver, hor = (torch.from_numpy(a).cuda() for a in (g, ver, hor))
        _CASES[key] = (g, ver, hor) + grad_input_ref64(g, ver, hor)
    return _CASES[key]


def _gi(g, ver, hor, algo=cunnex.ALGO_AUTO, taps=None, out=None, expect=0):
    """One C-ABI call.  grad_input starts as NaN, so an element the kernel does not write cannot pass any check below."""
    lib = sstem_native.load_library()
    B, C, H, W = g.shape
    K = ver.shape[1]
    if out is None:
        out = torch.full((B, C, H + K - 1, W + K - 1), float("nan"), device=g.device)
    assert g.is_contiguous() and ver.is_contiguous() and hor.is_contiguous() and out.is_contiguous()
    stream = torch.cuda.current_stream().cuda_stream
    if ver.dtype == torch.bfloat16:
        rc = lib.sstem_sepconv_backward_input_bf16coef(g.data_ptr(), ver.data_ptr(), hor.data_ptr(), out.data_ptr(), B, C, H, W, stream)
    elif taps is not None:
        rc = lib.sstem_sepconv_backward_input_taps_f32(g.data_ptr(), ver.data_ptr(), hor.data_ptr(), out.data_ptr(), B, C, H, W, taps, stream)
    else:
        rc = lib.sstem_sepconv_backward_input_f32_algo(g.data_ptr(), ver.data_ptr(), hor.data_ptr(), out.data_ptr(), B, C, H, W, stream, algo)
    assert rc == expect, (rc, lib.sstem_last_error().decode("utf-8", "replace"))
    torch.cuda.synchronize()
    return out


def _check(got, ref, S, family, what):
    worst = assert_within_rounding(got, ref, S, N_GRADINPUT, "%s [%s]" % (what, family))
    WORST[family] = max(WORST.get(family, 0.0), worst)
    print("%s [%s]: worst err / (2^-24 S) = %.2f" % (what, family, worst))


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 1 + 2: the bound at every element, both ids; tiled == direct bit for bit; each kernel repeats its bits ----------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_element_within_the_bound_for_both_ids(shape, kind):
    g, ver, hor, ref, S = _case(shape, kind)
    for algo, name in ALGOS:
        _check(_gi(g, ver, hor, algo), ref, S, "grad_input, " + name, "%s %s" % ("x".join(map(str, shape)), kind))
    _check(_gi(g, ver, hor), ref, S, "grad_input, auto", "%s %s" % ("x".join(map(str, shape)), kind))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tiled_equals_direct_bit_for_bit_and_both_repeat(shape, kind):
    g, ver, hor, _, _ = _case(shape, kind)
    d1, d2 = _gi(g, ver, hor, DIRECT), _gi(g, ver, hor, DIRECT)
    t1, t2 = _gi(g, ver, hor, MFMA), _gi(g, ver, hor, MFMA)
    assert _same_bits(d1, d2), "the direct kernel does not repeat its bits"
    assert _same_bits(t1, t2), "the tiled kernel does not repeat its bits"
    assert torch.equal(t1, d1), "tiled != direct: %d of %d elements differ, max |diff| %.3g" % (
        int((t1 != d1).sum()), d1.numel(), float((t1 - d1).abs().max()))


# ---- 3: grad_input fully overwritten, nothing around it touched ------------------------------------------------------------------------

@pytest.mark.parametrize("algo,name", ALGOS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_grad_input_is_fully_overwritten_and_nothing_else_is(shape, algo, name):
    g, ver, hor, ref, S = _case(shape, "randn")
    B, C, H, W = shape
    n = B * C * (H + 50) * (W + 50)
    front, back = 1031, 4099                                         # odd offsets: the slice is only 4-byte aligned
    SENT = 12345.0
    big = torch.full((front + n + back,), SENT, device="cuda")
    out = big[front:front + n].view(B, C, H + 50, W + 50)
    out.fill_(float("nan"))
    _gi(g, ver, hor, algo, out=out)
    assert torch.isfinite(out).all(), "%d elements of grad_input were not written" % int((~torch.isfinite(out)).sum())
    assert (big[:front] == SENT).all() and (big[front + n:] == SENT).all(), "a sentinel outside grad_input changed"
    _check(out, ref, S, "grad_input, " + name, "%s in guard bands" % "x".join(map(str, shape)))


# ---- 4: exact answers ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("algo,name", ALGOS)
def test_one_pixel_is_the_outer_product_in_the_stated_association(algo, name):
    g, ver, hor, _, _ = _case((1, 3, 1, 1), "randn")
    gh = g[0, :, 0, 0, None] * hor[0, None, :, 0, 0]                             # fl(g * H): one fp32 multiply  [C,fx]
    want = (ver[0, :, 0, 0].double()[None, :, None] * gh.double()[:, None, :]).float()   # fmaf(V, gh, +0) = fl(V * gh): exact product, one rounding
    got = _gi(g, ver, hor, algo)
    assert _same_bits(got[0], want)


PAIRS = [(0, 0), (50, 50), (0, 50), (50, 0), (25, 25), (7, 9)]


@pytest.mark.parametrize("algo,name", ALGOS)
@pytest.mark.parametrize("C,H,W", [(3, 15, 79), (1, 70, 30)])
def test_one_tap_pair_per_image_is_an_exact_shifted_copy(C, H, W, algo, name):
    B = len(PAIRS)
    g = torch.randn(B, C, H, W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    ver, hor = torch.zeros(B, 51, H, W, device="cuda"), torch.zeros(B, 51, H, W, device="cuda")
    want = torch.zeros(B, C, H + 50, W + 50, device="cuda")          # exact +0 everywhere else
    for b, (fy, fx) in enumerate(PAIRS):
        ver[b, fy], hor[b, fx] = 1.0, 1.0
        want[b, :, fy:fy + H, fx:fx + W] = g[b]
    got = _gi(g, ver, hor, algo)
    assert _same_bits(got, want), "%d elements differ in value or in the sign of zero" % int(
        (got.view(torch.int32) != want.view(torch.int32)).sum())


@pytest.mark.parametrize("algo,name", ALGOS)
def test_per_pixel_one_hot_taps_against_float64_index_put(algo, name):
    B, C, H, W = 2, 3, 37, 70
    _, ver, hor, g = make_case(31, B, C, H, W, "onehot")
    fy, fx = torch.from_numpy(ver.argmax(axis=1)).cuda(), torch.from_numpy(hor.argmax(axis=1)).cuda()      # [B,H,W]
    g, ver, hor = (torch.from_numpy(a).cuda() for a in (g, ver, hor))
    bb, cc, yy, xx = torch.meshgrid(*(torch.arange(n, device="cuda") for n in (B, C, H, W)), indexing="ij")
    idx = (bb, cc, yy + fy[:, None], xx + fx[:, None])
    ref = torch.zeros(B, C, H + 50, W + 50, dtype=torch.float64, device="cuda").index_put_(idx, g.double(), accumulate=True)
    S = torch.zeros_like(ref).index_put_(idx, g.double().abs(), accumulate=True)
    _check(_gi(g, ver, hor, algo), ref, S, "grad_input, " + name, "per-pixel one-hot taps")


# ---- 5: bf16 coefficients ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(2, 3, 37, 70), (1, 4, 20, 70)], ids=lambda s: "x".join(map(str, s)))
def test_bf16_entry_gives_the_f32_bits_on_the_widened_values(shape, kind):
    g, ver, hor, _, _ = _case(shape, kind)
    v16, h16 = ver.bfloat16(), hor.bfloat16()
    got = _gi(g, v16, h16)
    assert _same_bits(got, _gi(g, v16.float(), h16.float()))         # the _f32 entry (AUTO) on the widened tensors
    ref, S = grad_input_ref64(g, v16, h16)                           # the rounding to bf16 is the producer's
    _check(got, ref, S, "grad_input, bf16 coefficients", "%s %s" % ("x".join(map(str, shape)), kind))


# ---- 6: any filter length -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("taps", [5, 13])
def test_taps_entry(taps):
    B, C, H, W = 1, 2, 9, 11
    gen = torch.Generator(device="cuda").manual_seed(60 + taps)
    g = torch.randn(B, C, H, W, device="cuda", generator=gen)
    ver, hor = torch.randn(B, taps, H, W, device="cuda", generator=gen), torch.randn(B, taps, H, W, device="cuda", generator=gen)
    ref, S = grad_input_ref64(g, ver, hor, taps)
    _check(_gi(g, ver, hor, taps=taps), ref, S, "grad_input, %d taps" % taps, "1x2x9x11")


def test_taps_entry_with_51_taps_is_the_f32_entry():
    g, ver, hor, _, _ = _case((1, 3, 15, 79), "randn")
    assert _same_bits(_gi(g, ver, hor, taps=51), _gi(g, ver, hor))


def test_empty_image_sets_grad_input_to_zero():
    g = torch.zeros(2, 3, 0, 7, device="cuda")
    ver = hor = torch.zeros(2, 51, 0, 7, device="cuda")
    out = _gi(g, ver, hor)
    assert out.shape == (2, 3, 50, 57) and _same_bits(out, torch.zeros_like(out))


# ---- 7: autograd -------------------------------------------------------------------------------------------------------------------------

def _autograd_case():
    g, ver, hor, _, _ = _case((2, 3, 37, 70), "randn")
    inp = torch.rand(2, 3, 87, 120, device="cuda", generator=torch.Generator(device="cuda").manual_seed(70))
    return inp, ver, hor, g


def _grads(inp, ver, hor, g, inp_grad=True):
    i = inp.clone().requires_grad_(inp_grad)
    v, h = ver.clone().requires_grad_(), hor.clone().requires_grad_()
    out = SeparableConvolution.apply(i, v, h)
    return torch.autograd.grad(out, (i, v, h) if inp_grad else (v, h), g)


def test_switch_on_equals_the_c_abi_and_leaves_the_coefficient_gradients_alone():
    inp, ver, hor, g = _autograd_case()
    _, gv_off, gh_off = _grads(inp, ver, hor, g)
    with sepconv_pkg.input_gradient():
        gi, gv, gh = _grads(inp, ver, hor, g)
    assert _same_bits(gi, _gi(g, ver, hor))
    assert _same_bits(gv, gv_off) and _same_bits(gh, gh_off)
    assert gi.abs().max().item() > 0


def test_switch_on_honours_set_algorithm():
    inp, ver, hor, g = _autograd_case()
    with sepconv_pkg.input_gradient():
        for algo, _ in ALGOS:
            cunnex.set_algorithm(algo)
            gi, _, _ = _grads(inp, ver, hor, g)
            assert _same_bits(gi, _gi(g, ver, hor, algo))


def test_switch_off_gives_zeros():
    inp, ver, hor, g = _autograd_case()
    assert not sepconv_pkg.get_input_gradient()
    gi, _, _ = _grads(inp, ver, hor, g)
    assert gi.shape == inp.shape and _same_bits(gi, torch.zeros_like(gi))


def test_switch_on_returns_none_for_an_input_that_needs_no_gradient():
    inp, ver, hor, g = _autograd_case()

    class Ctx:
        saved_tensors = (inp, ver, hor)
        needs_input_grad = (False, True, True)

    _, gv_off, gh_off = _grads(inp, ver, hor, g)
    with sepconv_pkg.input_gradient():
        gi, gv, gh = SeparableConvolution.backward(Ctx, g)
        gv2, gh2 = _grads(inp, ver, hor, g, inp_grad=False)
    assert gi is None
    assert _same_bits(gv, gv_off) and _same_bits(gh, gh_off) and _same_bits(gv2, gv_off) and _same_bits(gh2, gh_off)


def test_context_manager_restores_the_state_after_an_exception():
    assert not sepconv_pkg.get_input_gradient()
    with pytest.raises(ZeroDivisionError):
        with sepconv_pkg.input_gradient():
            assert sepconv_pkg.get_input_gradient()
            1 / 0
    assert not sepconv_pkg.get_input_gradient()
    sepconv_pkg.set_input_gradient(True)
    with sepconv_pkg.input_gradient(False):
        assert not sepconv_pkg.get_input_gradient()
    assert sepconv_pkg.get_input_gradient()


def test_gradcheck_with_the_input_requiring_grad():
    """The reference's own tolerances (model_interp.py:109-119: eps=1e-2, atol=1e-2, rtol=1e-2), now with requires_grad=True on the
    input as well: B = 1, C = 2, input 51 x 51, coefficients [1,51,1,1] -- 5202 input elements."""
    torch.manual_seed(0)
    inputs = (torch.randn(1, 2, 51, 51).cuda().requires_grad_(),
              torch.randn(1, 51, 1, 1).cuda().requires_grad_(),
              torch.randn(1, 51, 1, 1).cuda().requires_grad_())
    with sepconv_pkg.input_gradient():
        assert torch.autograd.gradcheck(SeparableConvolution.apply, inputs, eps=1e-2, atol=1e-2, rtol=1e-2)


def test_function_sepconv_13_taps_input_gradient():
    B, C, H, W, taps = 1, 2, 9, 11, 13
    gen = torch.Generator(device="cuda").manual_seed(73)
    inp = torch.randn(B, C, H + taps - 1, W + taps - 1, device="cuda", generator=gen).requires_grad_()
    ver, hor = torch.randn(B, taps, H, W, device="cuda", generator=gen), torch.randn(B, taps, H, W, device="cuda", generator=gen)
    g = torch.randn(B, C, H, W, device="cuda", generator=gen)
    gi_off, = torch.autograd.grad(FunctionSepconv(inp, ver, hor), inp, g)
    assert _same_bits(gi_off, torch.zeros_like(gi_off))
    with sepconv_pkg.input_gradient():
        gi, = torch.autograd.grad(FunctionSepconv(inp, ver, hor), inp, g)
    ref, S = grad_input_ref64(g, ver, hor, taps)
    _check(gi, ref, S, "grad_input, FunctionSepconv 13 taps", "1x2x9x11")


# ---- 8: a chain that backpropagates through the frames ------------------------------------------------------------------------------------

def test_chain_through_pad_and_expand_and_its_gray_form():
    B, H, W = 2, 40, 72
    gen = torch.Generator(device="cuda").manual_seed(80)
    x = torch.randn(B, 1, H, W, device="cuda", generator=gen)
    ver, hor = torch.randn(B, 51, H, W, device="cuda", generator=gen), torch.randn(B, 51, H, W, device="cuda", generator=gen)
    pad = torch.nn.ReplicationPad2d(25)

    x64 = x.double().requires_grad_()
    patches = F.unfold(pad(x64.expand(B, 3, H, W)), kernel_size=51).view(B, 3, 51, 51, H, W)
    torch.einsum("bcijyx,biyx,bjyx->bcyx", patches, ver.double(), hor.double()).mean().backward()
    ref = x64.grad
    del patches

    with sepconv_pkg.input_gradient():
        xa = x.clone().requires_grad_()
        SeparableConvolution.apply(pad(xa.expand(B, 3, H, W)).contiguous(), ver, hor).mean().backward()
        xb = x.clone().requires_grad_()
        sepconv_gray(pad(xb).contiguous(), ver, hor).mean().backward()
    tol = 2e-5 * ref.abs().max().item()                              # the project's tolerance for random data
    ea, eb = (xa.grad.double() - ref).abs().max().item(), (xb.grad.double() - ref).abs().max().item()
    eab = (xa.grad.double() - xb.grad.double()).abs().max().item()
    print("chain: generic %.3g, gray %.3g, generic vs gray %.3g of max|ref|" % tuple(e / ref.abs().max().item() for e in (ea, eb, eab)))
    assert ref.abs().max().item() > 0
    assert ea <= tol and eb <= tol and eab <= tol


def test_sepconv_gray_forward_is_the_op_on_the_expanded_plane():
    B, H, W = 1, 15, 79
    gen = torch.Generator(device="cuda").manual_seed(81)
    plane = torch.rand(B, 1, H + 50, W + 50, device="cuda", generator=gen)
    ver, hor = torch.randn(B, 51, H, W, device="cuda", generator=gen), torch.randn(B, 51, H, W, device="cuda", generator=gen)
    want = SeparableConvolution.apply(plane.expand(B, 3, H + 50, W + 50).contiguous(), ver, hor)
    assert _same_bits(sepconv_gray(plane, ver, hor), want)
