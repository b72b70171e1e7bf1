"""Multi-pass row-pair form of the blocked fused apply (sepconv_gray_mfma_pair_hp, SSTEM_GRAY_PAIR=3) against the one-row kernel.

SSTEM_GRAY_PAIR: 0 = always the one-row kernel, 1 = the product default, 2 = always the row-pair kernel, 3 = always the multi-pass
row-pair kernel -- so every case below runs the new kernel, also where the default's grid gate would not pick it (the knob applies in
the launcher's 32-row family, which every shape here is large enough for).

The multi-pass kernel runs the same k-ordered MFMA chain per 4-row tile and the same fy-ascending vertical sum as the one-row kernel,
only in another order across tiles, so every output bit must agree.  The instances come from native_instances.py (one library copy
per knob setting) and run on the same device tensors through the C-ABI.
"""
import ctypes

import pytest
import torch

import sstem_native

pytestmark = pytest.mark.gpu

_BLOCKED = "sstem_sepconv_interp_apply_gray_blocked_f32"
_U8 = "sstem_sepconv_interp_apply_gray_u8_f32"


def _bind(lib):
    for name in (_BLOCKED, _U8):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = sstem_native.C_ABI[name]
    return lib


def _inst(pair):
    from native_instances import instance
    return _bind(instance(SSTEM_GRAY_PAIR=pair).lib)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _apply(lib, g1, g2, kb, u8=False, fill=None):
    B, _, H, W = g1.shape
    out = torch.empty(B, 1, H, W, device=g1.device)
    if fill is not None:
        out.fill_(fill)
    if u8:
        ob = torch.empty(B, H, W, dtype=torch.uint8, device=g1.device)
        rc = getattr(lib, _U8)(_p(g1), _p(g2), *(_p(k) for k in kb), _p(out), _p(ob), B, H, W, 1, _stream())
    else:
        ob = None
        rc = getattr(lib, _BLOCKED)(_p(g1), _p(g2), *(_p(k) for k in kb), _p(out), B, H, W, _stream())
    assert rc == 0, lib.sstem_last_error().decode("utf-8", "replace")
    torch.cuda.synchronize()
    return out, ob


def _case(B, H, W, seed):
    from libs.sepconv.fused import coef_to_blocked, coef_blocked_shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    g1 = torch.rand(B, 1, H, W, device="cuda", generator=g)
    g2 = torch.rand(B, 1, H, W, device="cuda", generator=g)
    if B * H * W > 4 * 1024 * 1024:          # C2: the blocked tensors directly (W = 1024: no padding columns)
        assert W % 64 == 0
        kb = [torch.rand(coef_blocked_shape(B, H, W), device="cuda", generator=g) / 25.5 for _ in range(4)]
    else:
        kb = [coef_to_blocked(torch.rand(B, 51, H, W, device="cuda", generator=g) / 25.5) for _ in range(4)]
    return g1, g2, kb


@pytest.mark.parametrize("B,H,W", [(8, 1024, 1024),     # C2, the bench.py launch
                                   (2, 1000, 1024),     # bottom tile of 40 rows: whole pairs
                                   (2, 1023, 1024),     # bottom tile of 63 rows: one wave ends on a half pair
                                   (2, 1024, 1000),     # partial last row segment
                                   (1, 1023, 1000),     # B = 1, both edges partial
                                   (2, 1026, 1024),     # bottom tile of 2 rows: two of its waves own no row at all
                                   (1, 1030, 1000)])    # bottom tile of 6 rows: two waves with a whole pair, two with a half pair
def test_halfpass_equals_one_row_kernel(B, H, W):
    g1, g2, kb = _case(B, H, W, 9001 + H + W)
    ref, _ = _apply(_inst(0), g1, g2, kb)
    got, _ = _apply(_inst(3), g1, g2, kb)
    assert torch.equal(got, ref), (B, H, W, (got - ref).abs().max().item())


@pytest.mark.parametrize("B,H,W", [(2, 1023, 1000), (1, 1000, 1024)])
def test_halfpass_u8_output_equals_one_row_kernel(B, H, W):
    g1, g2, kb = _case(B, H, W, 9200 + H)
    ref, ref_u8 = _apply(_inst(0), g1, g2, kb, u8=True)
    got, got_u8 = _apply(_inst(3), g1, g2, kb, u8=True)
    assert torch.equal(got, ref) and torch.equal(got_u8, ref_u8), (B, H, W)
    assert torch.equal(got_u8, (got[:, 0] * 255).to(torch.int64).to(torch.uint8))


@pytest.mark.parametrize("which", ["product", 2, 3])
def test_first_phase_does_not_read_the_output(which):
    """The first phase parks its channel sum in the output and only the second phase reads it back: whatever the output buffer held
    before the call (NaN here) must not reach the result.  `product` is the product library's own entry, whichever form it
    dispatches to; 2 and 3 force the two row-pair kernels."""
    g1, g2, kb = _case(2, 1023, 1024, 9300)
    ref, _ = _apply(_inst(0), g1, g2, kb)
    lib = _bind(sstem_native.load_library()) if which == "product" else _inst(which)
    got, _ = _apply(lib, g1, g2, kb, fill=float("nan"))
    assert torch.equal(got, ref), which
    got, got_u8 = _apply(lib, g1, g2, kb, u8=True, fill=float("nan"))
    assert torch.equal(got, ref), which
    assert torch.equal(got_u8, (ref[:, 0] * 255).to(torch.int64).to(torch.uint8))
