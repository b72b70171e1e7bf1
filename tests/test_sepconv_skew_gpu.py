"""B-operand skew of the blocked fused apply, checked against a gather -- no other kernel is the reference here.

The banded 4x4x1 formulation needs, in the lane at position j = lane & 3 of its 4-pixel block, raw[t - j] of its own pixel as entry t
of the B operand.  The kernels build that from the coalesced raw taps with selects (csrc/sepconv_kernels.hip: skew_taps_in_place, and
the two-select form p[t] = (j & 1) ? raw[t - 1] : raw[t], B[t] = (j >= 2) ? p[t - 2] : p[t] in sepconv_gray_mfma_pair_hp).  A slip
there moves a tap to a neighbouring one for some lane positions only, so the test makes every single tap visible on its own:

with H one-hot at tap fh and V one-hot at tap fv the apply is a pure gather,
    frame[clamp(y + fv - 25), clamp(x + fh - 25)]            (replication padding folded in),
every product is x * 1 or x * 0 and every sum adds zeros, so the output must equal, bit for bit, what torch computes in fp32 in the
kernel's own order: (((a + a) + a) + ((b + b) + b)) * float32(1 / 3) for the two frames' gathers a and b.  The pixels of an image cover
all four lane positions; fh = 0..50 covers both band edges (entries t < j and t >= 51 must come out as zeros).

The calls go through the C-ABI on instances from native_instances.py: SSTEM_GRAY_PAIR=0 (always the one-row kernel), =3 (always the
multi-pass row-pair kernel), and the product library's own dispatch.  The coefficient tensors are laid out in torch, not by the
library's layout kernel.
"""
import ctypes

import pytest
import torch

import sstem_native

pytestmark = pytest.mark.gpu

_BLOCKED = "sstem_sepconv_interp_apply_gray_blocked_f32"
F = 51

# (1, 1023, 1000): partial last row segment, bottom tile of 63 rows (one wave ends on a half pair); (2, 1030, 1024): two images, whole
# segments, bottom tile of 6 rows (two waves with a whole pair, two with a half pair)
SHAPES = [(1, 1023, 1000), (2, 1030, 1024)]
WHICH = [0, 3, "product"]


def _lib(which):
    if which == "product":
        lib = sstem_native.load_library()
    else:
        from native_instances import instance
        lib = instance(SSTEM_GRAY_PAIR=which).lib
    fn = getattr(lib, _BLOCKED)
    fn.restype, fn.argtypes = sstem_native.C_ABI[_BLOCKED]
    return lib


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _apply(lib, g1, g2, kb):
    B, _, H, W = g1.shape
    out = torch.full((B, 1, H, W), float("nan"), device=g1.device)
    rc = getattr(lib, _BLOCKED)(_p(g1), _p(g2), *(_p(k) for k in kb), _p(out), B, H, W,
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.sstem_last_error().decode("utf-8", "replace")
    torch.cuda.synchronize()
    return out


def _frames(B, H, W, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand(B, 1, H, W, device="cuda", generator=g), torch.rand(B, 1, H, W, device="cuda", generator=g))


def _one_hot_blocked(tap, B, H, W):
    """[B, H, ceil(W / 64), 51, 64] row-segment coefficients (include/sstem_sepconv.h): 1.0 at tap[b, y, x] of pixel (y, x), else 0.
    `tap` is an int64 [B, H, W] tensor; the padding columns of the last segment stay all zero."""
    S = (W + 63) // 64
    t = torch.full((B, H, S * 64), -1, dtype=torch.int64, device="cuda")
    t[:, :, :W] = tap
    k = torch.zeros(B, H, S, F, 64, device="cuda")
    t = t.view(B, H, S, 1, 64)
    k.scatter_(3, t.clamp(min=0), (t >= 0).float())
    return k


def _gather(frame, fv, fh):
    """frame[b, 0, clamp(y + fv - 25), clamp(x + fh - 25)] for int64 [B, H, W] tap tensors fv, fh."""
    B, _, H, W = frame.shape
    y = torch.arange(H, device="cuda").view(1, H, 1)
    x = torch.arange(W, device="cuda").view(1, 1, W)
    b = torch.arange(B, device="cuda").view(B, 1, 1)
    return frame[b, 0, (y + fv - F // 2).clamp(0, H - 1), (x + fh - F // 2).clamp(0, W - 1)].unsqueeze(1)


def _expected(g1, g2, taps):
    v1, h1, v2, h2 = taps
    a, b = _gather(g1, v1, h1), _gather(g2, v2, h2)
    return (((a + a) + a) + ((b + b) + b)) * torch.tensor(1.0 / 3, dtype=torch.float32, device="cuda")


def _check(lib, g1, g2, taps, what):
    B, _, H, W = g1.shape
    got = _apply(lib, g1, g2, [_one_hot_blocked(t.expand(B, H, W), B, H, W) for t in taps])
    want = _expected(g1, g2, taps)
    assert want.dtype == torch.float32
    bad = got != want                      # (NaN left in the output counts as different)
    if bad.any():
        where = bad.nonzero()[0].tolist()
        raise AssertionError("%s: %d of %d pixels differ, first at (b, c, y, x) = %s: got %r, want %r"
                             % (what, int(bad.sum()), bad.numel(), where, got[tuple(where)].item(), want[tuple(where)].item()))


@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("which", WHICH)
def test_every_horizontal_tap_alone_is_a_gather(which, B, H, W):
    """One tap for the whole image: every fh in 0..50, with a vertical tap that changes along (and the second frame at other taps)."""
    lib = _lib(which)
    g1, g2 = _frames(B, H, W, 4100 + H + W)
    for fh in range(F):
        taps = [torch.full((1, 1, 1), v, dtype=torch.int64, device="cuda") for v in ((7 * fh + 3) % F, fh, (11 * fh + 20) % F, F - 1 - fh)]
        _check(lib, g1, g2, taps, "which=%s fh=%d" % (which, fh))


@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("which", WHICH)
def test_per_pixel_taps_are_a_gather(which, B, H, W):
    """A tap index per pixel that differs between neighbouring pixels and rows (and images): the four lanes of a block then carry
    four different taps through the skew at once.  Several offsets, so that every pixel sees several of its taps."""
    lib = _lib(which)
    g1, g2 = _frames(B, H, W, 4200 + H + W)
    y = torch.arange(H, device="cuda").view(1, H, 1)
    x = torch.arange(W, device="cuda").view(1, 1, W)
    b = torch.arange(B, device="cuda").view(B, 1, 1)
    for off in (0, 1, 2, 3, 17, 48, 49, 50):
        taps = [((5 * x + 3 * y + 9 * b + off) % F).expand(B, H, W),
                ((x + 7 * y + 13 * b + off) % F).expand(B, H, W),          # neighbouring pixels: neighbouring taps, wrapping at 51
                ((2 * x + 11 * y + 4 * b + 2 * off) % F).expand(B, H, W),
                ((F - 1 - (3 * x + y + 5 * b + off) % F)).expand(B, H, W)]
        assert (taps[1][:, :, 1:] != taps[1][:, :, :-1]).all() and (taps[1][:, 1:] != taps[1][:, :-1]).all()
        _check(lib, g1, g2, taps, "which=%s off=%d" % (which, off))
