"""Row-pair form of the blocked fused apply (sepconv_gray_mfma_pair, SSTEM_GRAY_PAIR) against the one-row kernel it replaces.

SSTEM_GRAY_PAIR: 0 = always the one-row kernel, 1 = the product default (the pair form on grids of at least 512 of its workgroups),
2 = always the pair form -- so every case below runs the pair kernel at least once, small grids included.

Both kernels run the same k-ordered MFMA chains and the same fy-ascending vertical sum, so every output bit must agree.  The instances
come from native_instances.py (one library copy per knob setting) and run on the same device tensors through the C-ABI.
"""
import ctypes

import pytest
import torch

import sstem_native

pytestmark = pytest.mark.gpu

_BLOCKED = "sstem_sepconv_interp_apply_gray_blocked_f32"
_U8 = "sstem_sepconv_interp_apply_gray_u8_f32"


def _inst(pair):
    from native_instances import instance
    inst = instance(SSTEM_GRAY_PAIR=pair)
    for name in (_BLOCKED, _U8):
        fn = getattr(inst.lib, name)
        fn.restype, fn.argtypes = sstem_native.C_ABI[name]
    return inst


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _apply(inst, g1, g2, kb, u8=False):
    B, _, H, W = g1.shape
    out = torch.empty(B, 1, H, W, device=g1.device)
    if u8:
        ob = torch.empty(B, H, W, dtype=torch.uint8, device=g1.device)
        rc = getattr(inst.lib, _U8)(_p(g1), _p(g2), *(_p(k) for k in kb), _p(out), _p(ob), B, H, W, 1, _stream())
    else:
        ob = None
        rc = getattr(inst.lib, _BLOCKED)(_p(g1), _p(g2), *(_p(k) for k in kb), _p(out), B, H, W, _stream())
    assert rc == 0, inst.lib.sstem_last_error().decode("utf-8", "replace")
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
                                   (2, 1000, 1024),     # bottom tile of 8 rows: whole pairs
                                   (2, 1023, 1024),     # bottom tile of 31 rows: one wave ends on a half pair
                                   (2, 1024, 1000),     # partial last row segment
                                   (1, 1023, 1000)])    # B = 1, both edges partial
def test_rowpair_equals_one_row_kernel(B, H, W):
    g1, g2, kb = _case(B, H, W, 7001 + H + W)
    ref, _ = _apply(_inst(0), g1, g2, kb)
    for pair in (1, 2):
        got, _ = _apply(_inst(pair), g1, g2, kb)
        assert torch.equal(got, ref), (pair, B, H, W, (got - ref).abs().max().item())


def test_product_entry_equals_one_row_kernel():
    """interp_apply_gray_blocked (the product's inference entry, whichever form it dispatches to) gives the one-row kernel's bits."""
    from libs.sepconv.fused import interp_apply_gray_blocked
    g1, g2, kb = _case(2, 1023, 1000, 7100)
    ref, _ = _apply(_inst(0), g1, g2, kb)
    assert torch.equal(interp_apply_gray_blocked(g1, g2, *kb), ref)


@pytest.mark.parametrize("B,H,W", [(2, 1023, 1000), (1, 1000, 1024)])
def test_rowpair_u8_output_equals_one_row_kernel(B, H, W):
    g1, g2, kb = _case(B, H, W, 7200 + H)
    ref, ref_u8 = _apply(_inst(0), g1, g2, kb, u8=True)
    for pair in (1, 2):
        got, got_u8 = _apply(_inst(pair), g1, g2, kb, u8=True)
        assert torch.equal(got, ref) and torch.equal(got_u8, ref_u8), (pair, B, H, W)
        assert torch.equal(got_u8, (got[:, 0] * 255).to(torch.int64).to(torch.uint8))
