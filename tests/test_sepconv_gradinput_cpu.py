"""The sepconv input gradient without a GPU: the float64 reference against autograd, the adjoint identity against the C oracle, the
acceptance bound against an fp32 emulation of the kernels' order and four mutants of it, and the new C-ABI entries' argument handling.

Summation order under test (csrc/sepconv_kernels.h, include/sstem_sepconv.h): per grad_input element ONE chain from +0 over its source
pixels, rows ascending and columns ascending inside a row, each step  acc = fmaf(V, fl(g * H), acc).  n = N_GRADINPUT = 2610 is derived
in sepconv_gradinput_ref64's docstring (1 multiply + 2601 fmaf on the first term's path) and not tuned.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import libs.sepconv._ext.cunnex as cunnex
from oracle import sepconv_c
from sepconv_cases import make_case
from sepconv_gradinput_ref64 import N_GRADINPUT, grad_input_ref64
from sepconv_ref64 import rounding_report

NEW_SYMBOLS = ["sstem_sepconv_backward_input_f32", "sstem_sepconv_backward_input_f32_algo", "sstem_sepconv_backward_input_taps_f32",
               "sstem_sepconv_backward_input_bf16coef", "sstem_sepconv_backward_input_bytes"]


def _randn(seed, *shape):
    return torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


# ---- 1. the reference is the gradient ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("taps", [51, 5])
@pytest.mark.parametrize("B,C,H,W", [(1, 3, 37, 70), (2, 2, 5, 9)])
def test_reference_equals_autograd_through_an_independent_float64_forward(B, C, H, W, taps):
    inp = _randn(1, B, C, H + taps - 1, W + taps - 1).requires_grad_()
    ver, hor, g = _randn(2, B, taps, H, W), _randn(3, B, taps, H, W), _randn(4, B, C, H, W)
    patches = F.unfold(inp, kernel_size=taps).view(B, C, taps, taps, H, W)          # [b,c,fy,fx,y,x] = inp[b,c,y+fy,x+fx]
    out = torch.einsum("bcijyx,biyx,bjyx->bcyx", patches, ver, hor)
    want, = torch.autograd.grad(out, inp, g)
    ref, S = grad_input_ref64(g, ver, hor, taps)
    assert ref.shape == want.shape and ref.dtype == torch.float64
    err = (ref - want).abs().max().item()
    print("ref64 vs autograd %dx%dx%dx%d taps %d: max err / max|ref| = %.3g" % (B, C, H, W, taps, err / want.abs().max().item()))
    assert err <= 1e-12 * want.abs().max().item()
    assert (S >= ref.abs() * (1 - 1e-12)).all()
    # the four corners gather exactly one term
    assert S[0, 0, 0, 0].item() == abs(g[0, 0, 0, 0] * ver[0, 0, 0, 0] * hor[0, 0, 0, 0]).item()
    assert ref[0, 0, -1, -1].item() == pytest.approx((g[0, 0, -1, -1] * ver[0, -1, -1, -1] * hor[0, -1, -1, -1]).item(), rel=1e-15)


# ---- 2. adjoint identity with the C oracle's forward ----------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["softmax", "randn"])
def test_adjoint_identity_with_the_oracle_forward(kind):
    """<gI, r> = <g, forward(r, V, H)>, float64 dot products, the oracle's fp32 forward on the right.  Allowed difference: relative
    1e-5 of the dot product itself, the oracle's fp32 sums -- with positive data where nothing cancels (softmax coefficients, g > 0,
    r > 0) and with random signs (randn)."""
    B, C, H, W = 2, 3, 9, 14
    r, ver, hor, g = make_case(77, B, C, H, W, kind)
    if kind == "softmax":
        g = np.abs(g)
    fwd = sepconv_c.forward(r, ver, hor).astype(np.float64)
    gI, _ = grad_input_ref64(torch.from_numpy(g), torch.from_numpy(ver), torch.from_numpy(hor))
    left = float((gI * torch.from_numpy(r).double()).sum())
    right = float((g.astype(np.float64) * fwd).sum())
    scale = abs(right)
    print("adjoint %s: left %.12g right %.12g rel %.3g" % (kind, left, right, abs(left - right) / scale))
    assert abs(left - right) <= 1e-5 * scale


# ---- 3. the bound bites ------------------------------------------------------------------------------------------------------------------

def _emulate_fp32(g, ver, hor, mutant=None):
    """The kernels' order in fp32 with torch casts: source pixels (y, x) in row-major order, each adding its 51 x 51 window
    fmaf(V[fy], fl(g * H[fx]), acc) -- per target element that is the chain over its source rows, then columns, ascending.  The fused
    multiply-add is APPROXIMATED: the float64 product (exact for fp32 factors) plus the float64 accumulator, rounded to float64 and
    then to fp32 -- two roundings, which differ from a true fmaf by one fp32 ulp in rare near-ties; harmless for a bound check.
    mutant: "drop" one (fy, fx) pair everywhere, "transpose" the window, "late_clip" (source row H exists and reads row H-1),
    "other_image" (the other image's coefficients in the last 14 source rows)."""
    B, C, H, W = g.shape
    K = ver.shape[1]
    acc = torch.zeros(B, C, H + K - 1, W + K - 1, dtype=torch.float32)
    keep = torch.ones(K, K, dtype=torch.float64)
    if mutant == "drop":
        keep[7, 9] = 0.0
    rows = list(range(H)) + ([H] if mutant == "late_clip" else [])
    for y in rows:
        ys = min(y, H - 1)                                            # late_clip: the row past the end reads the last row
        vsrc, hsrc = ver, hor
        if mutant == "other_image" and y >= H - 14:
            vsrc, hsrc = ver.flip(0), hor.flip(0)
        for x in range(W):
            v = vsrc[:, :, ys, x]                                     # [B,K]
            gh = g[:, :, ys, x, None] * hsrc[:, None, :, ys, x]       # fp32 multiply: fl(g * H) [B,C,K]
            if mutant == "transpose":
                win = gh.double()[:, :, :, None] * v.double()[:, None, None, :]      # fy and fx swapped
            else:
                win = v.double()[:, None, :, None] * gh.double()[:, :, None, :]      # [B,C,fy,fx]
            tgt = acc[:, :, y:y + K, x:x + K]
            n_r = tgt.shape[2]                                        # late_clip: the window of row H is cut at the plane's end
            tgt.copy_((win[:, :, :n_r] * keep[:n_r] + tgt.double()).float())
    return acc


@pytest.fixture(scope="module")
def bound_case():
    B, C, H, W = 2, 3, 37, 70                                         # two images, so that "the other image" exists
    gen = torch.Generator().manual_seed(20)
    g = torch.randn(B, C, H, W, generator=gen)
    ver, hor = torch.randn(B, 51, H, W, generator=gen), torch.randn(B, 51, H, W, generator=gen)
    ref, S = grad_input_ref64(g, ver, hor)
    return g, ver, hor, ref, S


def test_the_implemented_order_stays_inside_the_bound(bound_case):
    g, ver, hor, ref, S = bound_case
    rep = rounding_report(_emulate_fp32(g, ver, hor), ref, S, N_GRADINPUT)
    print("fp32 emulation of the order: worst err / (2^-24 S) = %.2f of n = %d" % (rep["worst"], N_GRADINPUT))
    assert rep["bad"] == 0, rep
    assert rep["worst"] < N_GRADINPUT


@pytest.mark.parametrize("mutant", ["drop", "transpose", "late_clip", "other_image"])
def test_mutants_leave_the_bound_on_a_tenth_of_the_elements(bound_case, mutant):
    g, ver, hor, ref, S = bound_case
    rep = rounding_report(_emulate_fp32(g, ver, hor, mutant), ref, S, N_GRADINPUT)
    frac = rep["bad"] / ref.numel()
    print("mutant %-12s: %.1f %% of the elements outside %d * 2^-24 * S" % (mutant, 100 * frac, N_GRADINPUT))
    assert frac >= 0.10, (mutant, frac)


# ---- 4. the real library, no GPU ----------------------------------------------------------------------------------------------------------

def test_new_symbols_exist_and_are_bound():
    lib = cunnex.load_library()
    for name in NEW_SYMBOLS:
        assert name in cunnex.C_ABI, name
        assert hasattr(lib, name), name


def test_argument_handling_without_gpu():
    lib = cunnex.load_library()
    f32, algo = lib.sstem_sepconv_backward_input_f32, lib.sstem_sepconv_backward_input_f32_algo
    taps, bf16 = lib.sstem_sepconv_backward_input_taps_f32, lib.sstem_sepconv_backward_input_bf16coef
    nul = [None] * 4
    # a null pointer: 1; a negative size: 2; B == 0 (or C == 0): a successful no-op -- all before any HIP call
    assert f32(*nul, 1, 3, 4, 4, None) == 1
    assert algo(*nul, 1, 3, 4, 4, None, 2) == 1
    assert taps(*nul, 1, 3, 4, 4, 5, None) == 1
    assert bf16(*nul, 1, 3, 4, 4, None) == 1
    assert b"null" in lib.sstem_last_error()
    for bad in ((-1, 3, 4, 4), (1, -3, 4, 4), (1, 3, -4, 4), (1, 3, 4, -4)):
        assert f32(*nul, *bad, None) == 2
        assert algo(*nul, *bad, None, 1) == 2
        assert taps(*nul, *bad, 5, None) == 2
        assert bf16(*nul, *bad, None) == 2
    assert taps(*nul, 1, 3, 4, 4, 0, None) == 2                       # no filter
    assert f32(*nul, 0, 3, 4, 4, None) == 0
    assert algo(*nul, 0, 3, 4, 4, None, 2) == 0
    assert taps(*nul, 0, 3, 4, 4, 5, None) == 0
    assert bf16(*nul, 0, 3, 4, 4, None) == 0
    assert f32(*nul, 2, 0, 4, 4, None) == 0
    assert algo(*nul, 1, 3, 4, 4, None, 7) == 3                       # unknown algorithm id
    # H == 0: grad_input still has elements, so its pointer is needed
    assert f32(*nul, 1, 3, 0, 4, None) == 1


def test_byte_model():
    lib = cunnex.load_library()
    assert lib.sstem_sepconv_backward_input_bytes(8, 3, 1024, 1024) == 3633949056
    assert lib.sstem_sepconv_backward_input_bytes(8, 3, 1024, 1024) == lib.sstem_sepconv_forward_bytes(8, 3, 1024, 1024)


def test_switch_defaults_off_and_the_context_manager_restores_it():
    import libs.sepconv as pkg
    import os
    if not os.environ.get("SSTEM_SEPCONV_INPUT_GRAD"):
        assert pkg.get_input_gradient() is False                      # the variable is read once at import; unset: off
    pkg.set_input_gradient(False)
    with pkg.input_gradient():
        assert pkg.get_input_gradient() is True
        with pkg.input_gradient(False):
            assert pkg.get_input_gradient() is False
        assert pkg.get_input_gradient() is True
    assert pkg.get_input_gradient() is False
    with pytest.raises(KeyError):
        with pkg.input_gradient():
            raise KeyError("x")
    assert pkg.get_input_gradient() is False
    assert callable(pkg.set_input_gradient) and callable(pkg.sepconv_gray)
