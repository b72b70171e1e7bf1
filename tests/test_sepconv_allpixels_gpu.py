"""Every pixel of the sepconv kernels against the float64 reference of tests/sepconv_ref64.py, at the shapes where the launchers'
gates switch kernels and where tiles, row pairs and 4-pixel blocks end inside the image.

The other sepconv GPU tests prove "the same bits as the one-row kernel" and "a one-hot tap is a gather", and compare dense
coefficients with the serial C oracle on small shapes and three crops of one 8 x 1024 x 1024 tensor.  Here the reference is computed
on the GPU itself (F.pad + 2601 shifted float64 multiply-adds: nothing shared with the kernels), so every output element of every case
is held to  |got - ref| <= n * 2^-24 * S  (n = 110 apply / forward, 161 gradients: derived in sepconv_ref64's docstring, not tuned).
The project's older bounds (2e-5 of max|ref|; 1e-4 absolute on softmax coefficients) stay as second assertions.

Gates of the blocked fused apply (launch_gray<2, true> in csrc/sepconv_kernels.hip), with tx = ceil(W/64):
    T64 = B * tx * ceil(H/64),  T32 = B * tx * ceil(H/32)
    T64 >= 512                -> sepconv_gray_mfma_pair_hp<4,16,2>           ("pair_hp", 64-row tiles)
    T64 <  512 and T32 >= 512 -> sepconv_gray_mfma<2,4,8,3,false,2,true>     ("one-row 32", 32-row tiles)
    T32 <  512                -> sepconv_gray_mfma<2,4,4,3,false,2,true>     ("one-row 16", 16-row tiles)
SSTEM_GRAY_PAIR (0 one-row, 2 group-by-group pair, 3 multi-pass pair) acts only where T32 >= 512.

Each test prints the worst err / (2^-24 S) it saw, per kernel family (run with -s; DESIGN.md section 3 records them).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import sstem_native
from libs.sepconv.SeparableConvolution import SeparableConvolution
from libs.sepconv.fused import (coef_blocked_shape, coef_to_blocked, interp_apply, interp_apply_gray, interp_apply_gray_bf16coef,
                                interp_apply_gray_blocked, interp_apply_gray_blocked_supported, interp_apply_gray_supported,
                                interp_apply_gray_u8)
from sepconv_ref64 import N_APPLY, N_GRAD, apply_ref64, assert_within_rounding, backward_ref64, forward_ref64

pytestmark = pytest.mark.gpu
REL, ABS = 2e-5, 1e-4
KINDS = ["randn", "softmax"]
_BLOCKED = "sstem_sepconv_interp_apply_gray_blocked_f32"
_GRAY = "sstem_sepconv_interp_apply_gray_f32"
WORST = {}


@pytest.fixture(autouse=True)
def _free_between_cases():
    yield
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for family in sorted(WORST):
        print("\nWORST err / (2^-24 S)  %-40s %8.2f" % (family, WORST[family]))


def _check(got, ref, S, n, family, what, kind=None, second=True):
    """The derived bound at every element; then the project's older bounds; records the worst ratio of the family."""
    worst = assert_within_rounding(got, ref, S, n, "%s [%s]" % (what, family))
    WORST[family] = max(WORST.get(family, 0.0), worst)
    print("%s [%s]: worst err / (2^-24 S) = %.2f" % (what, family, worst))
    if second:
        err = (got.double() - ref).abs().max().item()
        assert err <= REL * ref.abs().max().item(), (what, err, ref.abs().max().item())
        if kind == "softmax" and n == N_APPLY:
            assert err <= ABS, (what, err)
    return worst


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _coef(g, B, H, W, kind):
    k = torch.randn(B, 51, H, W, device="cuda", generator=g)
    return torch.softmax(k, dim=1) if kind == "softmax" else k


def _apply_case(seed, B, H, W, kind):
    g = _gen(seed)
    g1 = torch.rand(B, 1, H, W, device="cuda", generator=g)
    g2 = torch.rand(B, 1, H, W, device="cuda", generator=g)
    return g1, g2, [_coef(g, B, H, W, kind) for _ in range(4)]          # k1v, k1h, k2v, k2h


def _gates(B, H, W):
    tx = (W + 63) // 64
    t64, t32 = B * tx * ((H + 63) // 64), B * tx * ((H + 31) // 32)
    return t64, t32, ("pair_hp" if t64 >= 512 else "one-row 32" if t32 >= 512 else "one-row 16")


def _inst(pair):
    from native_instances import instance
    inst = instance(SSTEM_GRAY_PAIR=pair)
    fn = getattr(inst.lib, _BLOCKED)
    fn.restype, fn.argtypes = sstem_native.C_ABI[_BLOCKED]
    return inst


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _forced_blocked(pair, g1, g2, kb):
    inst = _inst(pair)
    B, _, H, W = g1.shape
    out = torch.empty(B, 1, H, W, device=g1.device)
    rc = getattr(inst.lib, _BLOCKED)(_p(g1), _p(g2), *(_p(k) for k in kb), _p(out), B, H, W,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, inst.lib.sstem_last_error().decode("utf-8", "replace")
    torch.cuda.synchronize()
    return out


# ---- blocked fused apply on the product dispatch --------------------------------------------------------------------------------------
# (B, H, W, T64, T32, the kernel the gates pick)
BLOCKED_SHAPES = [
    (8, 1024, 1024, 2048, 4096, "pair_hp"),      # T64 = 8*16*16 = 2048: pair_hp, the benchmark launch, all 8.4 M pixels
    (32, 256, 256, 512, 1024, "pair_hp"),        # T64 = 32*4*4 = 512: pair_hp exactly at its gate
    (31, 256, 256, 496, 992, "one-row 32"),      # T64 = 496 < 512, T32 = 31*4*8 = 992: the one-row kernel, just below the gate
    (64, 256, 256, 1024, 2048, "pair_hp"),       # T64 = 64*4*4 = 1024: pair_hp, the 256 x 256 production size
    (16, 256, 256, 256, 512, "one-row 32"),      # T64 = 256, T32 = 16*4*8 = 512: the 32-row one-row kernel at its own gate
    (15, 256, 256, 240, 480, "one-row 16"),      # T64 = 240, T32 = 480 < 512: the 16-row small-grid shape
    (512, 40, 64, 512, 1024, "pair_hp"),         # T64 = 512*1*1: pair_hp, one 40-row tile per image, top and bottom padding in one tile
    (256, 70, 100, 1024, 1536, "pair_hp"),       # T64 = 256*2*2: pair_hp, bottom tile of 6 rows, last segment of 36 columns
    (2, 1027, 1021, 544, 1056, "pair_hp"),       # T64 = 2*16*17 = 544: pair_hp, W = 1 (mod 4), bottom tile of 3 rows (T32 = 2*16*33)
    (2, 1025, 1023, 544, 1056, "pair_hp"),       # T64 = 2*16*17 = 544: pair_hp, W = 3 (mod 4), bottom tile of 1 row
    (1, 1030, 999, 272, 528, "one-row 32"),      # T64 = 1*16*17 = 272, T32 = 16*33 = 528: one-row in the product; pair forms forced below
]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,H,W,t64,t32,kernel", BLOCKED_SHAPES)
def test_blocked_apply_every_pixel(B, H, W, t64, t32, kernel, kind):
    assert _gates(B, H, W) == (t64, t32, kernel)                     # the table above says what launch_gray<2, true> does
    assert interp_apply_gray_blocked_supported(B, H, W)
    g1, g2, ks = _apply_case(9000 + 7 * B + H + W, B, H, W, kind)
    kb = [coef_to_blocked(k) for k in ks]
    ref, S = apply_ref64(g1, g2, *ks)                                # from the NCHW tensors: independent of coef_to_blocked
    what = "blocked apply %dx%dx%d %s" % (B, H, W, kind)
    out = interp_apply_gray_blocked(g1, g2, *kb)                     # the product dispatch
    _check(out, ref, S, N_APPLY, "fused apply, blocked, " + kernel, what + " (product)", kind)
    if t32 >= 512:                                                   # where SSTEM_GRAY_PAIR applies: every form, forced
        del ks
        forced = {}
        for pair, name in ((0, "one-row 32"), (2, "pair"), (3, "pair_hp")):
            forced[pair] = _forced_blocked(pair, g1, g2, kb)
            _check(forced[pair], ref, S, N_APPLY, "fused apply, blocked, " + name, what + " (SSTEM_GRAY_PAIR=%d)" % pair, kind)
        assert torch.equal(forced[0], forced[2]) and torch.equal(forced[0], forced[3])
        assert torch.equal(out, forced[0])


# ---- the other entries of the apply ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,H,W,family", [
    (4, 1024, 1024, "NCHW gray, 64-row"),        # T64 = 4*16*16 = 1024: sepconv_gray_mfma<2,4,16,2,true,2> (shape 3) at its gate
    (3, 1000, 1021, "NCHW gray, 32-row"),        # T64 = 3*16*16 = 768 < 1024, T32 = 3*16*32 = 1536: shape 0, W = 1 (mod 4)
    (15, 256, 256, "NCHW gray, 16-row"),         # T32 = 15*4*8 = 480 < 512: shape 7
])
def test_nchw_gray_apply_every_pixel(B, H, W, family, kind):
    assert interp_apply_gray_supported(B, H, W)
    g1, g2, ks = _apply_case(9100 + B + H + W, B, H, W, kind)
    ref, S = apply_ref64(g1, g2, *ks)
    _check(interp_apply_gray(g1, g2, *ks), ref, S, N_APPLY, "fused apply, " + family, "gray apply %dx%dx%d %s" % (B, H, W, kind), kind)


def _apply_rgb_ref64(i1, i2, k1v, k1h, k2v, k2h):
    """model_interp.py:90-97 on frames with three different channels: the channel mean of the two images' sums.  The kernel spends
    51 + 51 fma, the other image's add, (o0 + o1) + o2 and the multiply by float32(1/3) on every term: N_APPLY covers it."""
    pad = lambda t: F.pad(t, (25, 25, 25, 25), mode="replicate")
    r2, s2 = forward_ref64(pad(i2), k2v, k2h)
    r1, s1 = forward_ref64(pad(i1), k1v, k1h)
    return (r2 + r1).sum(dim=1, keepdim=True) / 3.0, (s2 + s1).sum(dim=1, keepdim=True) / 3.0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,H,W", [(2, 1027, 1021), (3, 250, 250)])
def test_rgb_apply_every_pixel(B, H, W, kind):
    """interp_apply on frames whose channels differ: the device-side dispatch sends them to sepconv_rgb_stream_mfma<2, 8, 4>."""
    g = _gen(9200 + B + H + W)
    i1 = torch.rand(B, 3, H, W, device="cuda", generator=g)
    i2 = torch.rand(B, 3, H, W, device="cuda", generator=g)
    ks = [_coef(g, B, H, W, kind) for _ in range(4)]
    ref, S = _apply_rgb_ref64(i1, i2, *ks)
    _check(interp_apply(i1, i2, *ks), ref, S, N_APPLY, "fused apply, RGB stream", "rgb apply %dx%dx%d %s" % (B, H, W, kind), kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,H,W", [(2, 1027, 1021),      # T32 = 2*16*33 = 1056: sepconv_gray_mfma<2,4,8,3,false,2,false,true>
                                   (15, 256, 256)])      # T32 = 480 < 512: the 16-row form <2,4,4,3,false,2,false,true>
def test_bf16coef_apply_every_pixel(B, H, W, kind):
    g1, g2, ks = _apply_case(9300 + B + H + W, B, H, W, kind)
    k16 = [k.bfloat16() for k in ks]
    del ks
    ref, S = apply_ref64(g1, g2, *k16)                               # on the widened values: the rounding to bf16 is the producer's
    _check(interp_apply_gray_bf16coef(g1, g2, *k16), ref, S, N_APPLY, "fused apply, bf16 coefficients",
           "bf16coef apply %dx%dx%d %s" % (B, H, W, kind), kind)


@pytest.mark.parametrize("kind", KINDS)
def test_u8_apply_every_pixel_both_layouts(kind):
    B, H, W = 2, 1025, 1023                                          # blocked: T64 = 544, pair_hp; NCHW: T32 = 1056, shape 0
    g1, g2, ks = _apply_case(9400, B, H, W, kind)
    ref, S = apply_ref64(g1, g2, *ks)
    for layout, coefs in (("NCHW", ks), ("blocked", [coef_to_blocked(k) for k in ks])):
        out, img = interp_apply_gray_u8(g1, g2, *coefs)
        _check(out, ref, S, N_APPLY, "fused apply, uint8 store, " + layout, "u8 apply %s %s" % (layout, kind), kind)
        assert torch.equal(img, (out[:, 0] * 255).to(torch.int64).to(torch.uint8)), layout


# ---- forward op and both gradients ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("gray", [True, False], ids=["gray", "rgb"])
@pytest.mark.parametrize("B,H,W,size", [
    (4, 1024, 1024, "64-row"),       # T64 = 4*16*16 = 1024: forward shape 3, gradVertical shape 1, gradHorizontal shape 3, each at its gate
    (3, 1000, 1021, "32-row"),       # T64 = 768: the shapes below the gates (forward 0, gradVertical 0, gradHorizontal 2)
    (2, 250, 250, "16-row"),         # T32 = 2*4*8 = 64 < 512: the small-grid forward (shape 7)
])
def test_forward_and_gradients_every_element(B, H, W, size, gray, kind):
    g = _gen(9500 + B + H + W + int(gray))
    if gray:
        inp = torch.rand(B, 1, H + 50, W + 50, device="cuda", generator=g).expand(B, 3, H + 50, W + 50).contiguous()
    else:
        inp = torch.rand(B, 3, H + 50, W + 50, device="cuda", generator=g)
    ver, hor = _coef(g, B, H, W, kind), _coef(g, B, H, W, kind)
    grad = torch.randn(B, 3, H, W, device="cuda", generator=g)       # three different gradient channels
    v, h = ver.clone().requires_grad_(), hor.clone().requires_grad_()
    out = SeparableConvolution.apply(inp, v, h)
    out.backward(grad)
    out, gv, gh = out.detach(), v.grad, h.grad
    del v, h
    fam = ("gray, " if gray else "RGB, ") + size
    what = "%dx3x%dx%d %s %s" % (B, H, W, "gray" if gray else "rgb", kind)
    ref, S = forward_ref64(inp, ver, hor)
    _check(out, ref, S, N_APPLY, "forward op, " + fam, "forward " + what, kind)
    del ref, S, out
    rv, rh, Sv, Sh = backward_ref64(grad, inp, ver, hor)
    _check(gv, rv, Sv, N_GRAD, "gradVertical, " + fam, "gradVertical " + what)
    del rv, Sv, gv
    _check(gh, rh, Sh, N_GRAD, "gradHorizontal, " + fam, "gradHorizontal " + what)


# ---- one image whose coefficients end 16.8 MB below 4 GiB -----------------------------------------------------------------------------

def test_apply_near_the_4gib_limit_every_pixel_and_refusal_beyond_it():
    """One 4096 x 5120 image: its NCHW coefficients (51 * 4096 * 5120 * 4 B) and its blocked coefficients (4096 * 80 * 51 * 256 B) are
    4 278 190 080 bytes each, 16.8 MB below 2^32, so the scalar offsets of the last rows exceed 2^31 behind the kernels' 32-bit buffer
    resources.  Both _supported() calls answer 1; the blocked apply (pair_hp: T64 = 80 * 64 = 5120) and the NCHW gray apply (64-row
    shape) are checked at all 21 M pixels, softmax coefficients.  Each coefficient tensor is generated once, in the blocked layout; the
    NCHW tensors are its gathered copy and the reference reads the blocked ones through a permuted view.
    Peak device memory: 4 x 4.28 GB blocked + 4 x 4.28 GB NCHW + one softmax / gather transient and the reference's 2 GB of chunk
    temporaries = about 41 GB by this count (the measured peak is printed and asserted below 48 GB).
    One row segment beyond the limit (blocked: 328 966 segments of 13 056 B; NCHW: 21 053 762 pixels) _supported() answers 0 and the
    entry returns SSTEM_ERR_UNSUPPORTED before it launches anything."""
    lib = sstem_native.load_library()
    B, H, W = 1, 4096, 5120
    nbytes = 51 * H * W * 4
    assert nbytes == 4278190080 and 4096 * 80 * 51 * 256 == nbytes and (1 << 31) < nbytes < (1 << 32)
    assert lib.sstem_sepconv_interp_apply_gray_supported(B, H, W) == 1
    assert lib.sstem_sepconv_interp_apply_gray_blocked_supported(B, H, W) == 1

    # beyond the limit: refused without a launch (the tiny tensors below are never touched: the check precedes the launch)
    assert lib.sstem_sepconv_interp_apply_gray_blocked_supported(1, 328965, 64) == 1      # 328965 * 13056 = 4 294 967 040 < 2^32
    assert lib.sstem_sepconv_interp_apply_gray_blocked_supported(1, 328966, 64) == 0      # one row segment more
    assert lib.sstem_sepconv_interp_apply_gray_supported(1, 21053761, 1) == 1             # 51 * 4 * 21053761 = 2^32 - 52
    assert lib.sstem_sepconv_interp_apply_gray_supported(1, 21053762, 1) == 0
    tiny = torch.zeros(64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name, (h, w) in ((_BLOCKED, (328966, 64)), (_GRAY, (21053762, 1))):
        rc = getattr(lib, name)(*[_p(tiny)] * 7, 1, h, w, stream)
        assert rc == 3, (name, rc)                                                         # SSTEM_ERR_UNSUPPORTED
        assert b"4 GiB" in lib.sstem_last_error()
    torch.cuda.synchronize()
    assert tiny.abs().max().item() == 0.0

    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    g = _gen(9900)
    g1 = torch.rand(B, 1, H, W, device="cuda", generator=g)
    g2 = torch.rand(B, 1, H, W, device="cuda", generator=g)
    assert coef_blocked_shape(B, H, W) == (1, 4096, 80, 51, 64)      # W = 80 * 64: no padding pixels
    kb = []
    for _ in range(4):
        k = torch.randn(coef_blocked_shape(B, H, W), device="cuda", generator=g)
        kb.append(torch.softmax(k, dim=3))
        del k
    out_b = interp_apply_gray_blocked(g1, g2, *kb)
    torch.cuda.synchronize()
    views = [k.permute(0, 3, 1, 2, 4) for k in kb]                   # [1,51,H,80,64]: what the reference reads, no copy
    ks = [v.reshape(B, 51, H, W) for v in views]                     # the same values as NCHW tensors (a gather)
    assert all(k.is_contiguous() and k.data_ptr() != b.data_ptr() for k, b in zip(ks, kb))
    out_n = interp_apply_gray(g1, g2, *ks)
    torch.cuda.synchronize()
    ref, S = apply_ref64(g1, g2, *views)
    _check(out_b, ref, S, N_APPLY, "fused apply near 4 GiB, blocked pair_hp", "blocked apply 1x4096x5120 softmax", "softmax")
    _check(out_n, ref, S, N_APPLY, "fused apply near 4 GiB, NCHW gray 64-row", "gray apply 1x4096x5120 softmax", "softmax")
    # the last rows are the ones behind offsets >= 2^31: say so, so that the every-pixel check above is known to cover them
    assert (H - 1) * 80 * 51 * 256 >= 1 << 31 and 50 * H * W * 4 >= 1 << 31
    peak = torch.cuda.max_memory_allocated()
    print("near-4-GiB case: peak device memory %.1f GB" % (peak / 1e9))
    assert peak < 48e9
