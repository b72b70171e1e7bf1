"""Every element of the streaming kernels (csrc/misc_kernels.hip, csrc/warp_kernels.hip) against the float64 references of
tests/stream_ref64.py, at the shapes where their launchers switch code paths: the plane walks of the four up-sampling kernels, the
65535-row cap, ragged tiles in both directions, the grid-stride wraps of the warp, Adam, pooling and the uint8 edge, and pooling's
pointer gate.

The references are computed on the GPU itself from a device generator.  Up-sampling and Adam are held to the derived rounding bounds
|got - ref| <= n * 2^-24 * S  (N_UP = 5, N_UP_BWD = 15, N_ADAM_M = 5, N_ADAM_V = 6, and the composite S_p of Adam's parameter: derived in
stream_ref64's docstring, not tuned); the warp, pooling and the uint8 edge are held bit for bit.

Gates of launch_upsample_bilinear2x, restated by ``_which`` (OW = 2W, OH = 2H; every count below is asserted):
    OW >= 256 (and SSTEM_UPSAMPLE_WIDE != 0)   wide<TXL>, TXL = 256 / 128 / 64 from OW >= 1024 / 512 / below; tiles of 4 TXL columns x 1024 / TXL rows;
                                               grid rows = planes, or ceil(4096 / tiles) once tiles * planes > 4096 (the plane walk)
    OW >= 128                                  tiled; tiles of 256 columns x 4 rows; the walk starts at tiles * planes > 16384
    below                                      4-per-thread; gx = ceil(OH * (OW / 4) / 256); the walk starts at gx * planes > 65536, capped at 65535 rows
and of launch_upsample_bilinear2x_backward (``_which_bwd``): tiles of 64 x 4 / 32 x 8 / 16 x 16 input pixels from W >= 64 / 32 / below; the
walk starts at tiles * planes > 16384.

Each test prints the worst err / (2^-24 S) it saw, per kernel family (run with -s; DESIGN.md section 3 records them).
"""
import ctypes

import numpy as np
import pytest
import torch

import sstem_native
from stream_ref64 import (N_ADAM_M, N_ADAM_P, N_ADAM_V, N_UP, N_UP_BWD, adam_inputs, adam_ref64, assert_within_rounding, f32_to_u8_ref,
                          upsample2x_backward_ref64, upsample2x_ref64)

pytestmark = pytest.mark.gpu
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


def _check(got, ref, S, n, family, what):
    worst = assert_within_rounding(got, ref, S, n, "%s [%s]" % (what, family))
    WORST[family] = max(WORST.get(family, 0.0), worst)
    print("%s [%s]: worst err / (2^-24 S) = %.2f" % (what, family, worst))
    return worst


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _call(lib, name, *args):
    rc = getattr(lib, name)(*args, _stream())
    assert rc == 0, (name, rc, lib.sstem_last_error().decode("utf-8", "replace"))
    torch.cuda.synchronize()


def _ceil(a, b):
    return (a + b - 1) // b


# ---- up-sampling forward ----------------------------------------------------------------------------------------------------------------

def _which(planes, H, W, wide=1):
    """(kernel, grid x, grid y) of launch_upsample_bilinear2x; the workgroups walk planes where grid y < planes."""
    OH, OW = 2 * H, 2 * W
    if wide and OW >= 256 and OW % 4 == 0 and H * W < 1 << 29:
        txl = 256 if OW >= 1024 else (128 if OW >= 512 else 64)
        tiles = _ceil(OW, 4 * txl) * _ceil(OH, 4 * (256 // txl))
        gy = planes if tiles * planes <= 4096 else _ceil(4096, tiles)
        return "wide<%d>" % txl, tiles, max(1, min(gy, 65535))
    if OW >= 128 and H * W < 1 << 29:
        tiles = _ceil(OW, 256) * _ceil(OH, 4)
        gy = planes if tiles * planes <= 16384 else _ceil(16384, tiles)
        return "tiled", tiles, max(1, min(gy, 65535))
    gx = _ceil(OH * (OW // 4), 256)
    gy = planes if gx * planes <= 65536 else _ceil(65536, gx)
    return "4-per-thread", gx, max(1, min(gy, 65535))


# (planes, H, W, kernel, grid x, grid y)
FORWARD_CASES = [
    (3, 5, 6, "4-per-thread", 1, 3),              # OW = 12: 10 rows x 3 groups = 30 threads of one workgroup; the 16-byte source load only where xlo + 3 < 6
    (2, 1, 2, "4-per-thread", 1, 2),              # one source row (ry = 0), one group per output row, every source read clamped
    (5, 7, 62, "4-per-thread", 2, 5),             # OW = 124, the widest below the tiled gate: 14 x 31 = 434 threads, the second workgroup ragged
    (70000, 8, 8, "4-per-thread", 1, 65535),      # gx = 1: 70000 > 65536 -> 65536 rows, capped at 65535: planes 0 .. 4464 share a thread with plane + 65535
    (3, 3, 64, "tiled", 2, 3),                    # OW = 128, exactly at the gate: one half-used 256-column tile, OH = 6 = a full and a 2-row tile
    (2, 33, 126, "tiled", 17, 2),                 # OW = 252 of 256 columns, OH = 66: the 17th tile has 2 rows
    (9000, 3, 66, "tiled", 2, 8192),              # 2 tiles * 9000 = 18000 > 16384: 8192 grid rows, planes 0 .. 807 walk to plane + 8192
    (1100, 9, 130, "wide<64>", 4, 1024),          # OW = 260 = 256 + 4, OH = 18 = 16 + 2: 2 x 2 tiles, ragged both ways; 4400 > 4096: 1024 rows, 76 walk
    (1100, 5, 258, "wide<128>", 4, 1024),         # OW = 516 = 512 + 4, OH = 10 = 8 + 2
    (1100, 3, 514, "wide<256>", 4, 1024),         # OW = 1028 = 1024 + 4, OH = 6 = 4 + 2
]


def _upsample(x):
    import hipnn.functional as HF
    out = HF.upsample_bilinear2x(x[None])[0]
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("planes,H,W,kernel,gx,gy", FORWARD_CASES)
def test_upsample_forward_every_element(planes, H, W, kernel, gx, gy):
    assert _which(planes, H, W) == (kernel, gx, gy)
    x = torch.randn(planes, H, W, device="cuda", generator=_gen(1000 + planes + H + W))
    out = _upsample(x)
    ref, S = upsample2x_ref64(x)
    _check(out, ref, S, N_UP, "up-sampling forward, " + kernel, "%dx%dx%d" % (planes, H, W))


@pytest.mark.parametrize("planes,H,W,wide_grid,tiled_grid", [
    (2, 37, 1030, ("wide<256>", 57, 2), ("tiled", 171, 2)),       # OW = 2060: 3 x 19 wide tiles (the third 12 columns, the 19th 2 rows); 9 x 19 tiled
                                                                   # tiles, the ninth 12 columns wide, its staging window clamped to column 1029
    (1, 250, 512, ("wide<256>", 125, 1), ("tiled", 500, 1)),      # the 512 x 512 planes of the kernel heads: whole tiles only
])
def test_upsample_forward_wide_and_tiled_kernels_each_against_the_reference(planes, H, W, wide_grid, tiled_grid, monkeypatch):
    assert _which(planes, H, W, 1) == wide_grid and _which(planes, H, W, 0) == tiled_grid
    x = torch.randn(planes, H, W, device="cuda", generator=_gen(1100 + W))
    ref, S = upsample2x_ref64(x)
    wide = _upsample(x)
    monkeypatch.setenv("SSTEM_UPSAMPLE_WIDE", "0")                # read per launch
    tiled = _upsample(x)
    monkeypatch.delenv("SSTEM_UPSAMPLE_WIDE")
    _check(wide, ref, S, N_UP, "up-sampling forward, wide<256>", "%dx%dx%d" % (planes, H, W))
    _check(tiled, ref, S, N_UP, "up-sampling forward, tiled", "%dx%dx%d (SSTEM_UPSAMPLE_WIDE=0)" % (planes, H, W))
    assert torch.equal(wide, tiled)


@pytest.mark.parametrize("planes,H,W", [(3, 4, 64), (3, 4, 128), (2, 33, 126)])
def test_upsample_forward_three_kernels_same_bits(planes, H, W, monkeypatch):
    """The 4-per-thread kernel takes any even width, so a private instance of the library with the tiled kernels switched off
    (SSTEM_UPSAMPLE_TILED=0, read once per instance) runs it on the very planes the tiled and the wide kernel take: the same bits from
    all that apply (lerp2 spells the rounding out).  Planes of DIFFERENT widths share no outputs -- the scale (W - 1) / (2W - 1)
    differs -- so (3,4,62) has no partner; its kernel is compared here at 64, 126 and 128 columns instead."""
    from native_instances import instance
    x = torch.randn(planes, H, W, device="cuda", generator=_gen(1200 + W))
    ref, S = upsample2x_ref64(x)
    product = _upsample(x)                                         # the shared library has read its own knobs before the variable exists
    monkeypatch.setenv("SSTEM_UPSAMPLE_TILED", "0")
    inst = instance(SSTEM_UPSAMPLE_TILED=0)
    fn = inst.lib.sstem_upsample_bilinear2x_f32
    fn.restype, fn.argtypes = sstem_native.C_ABI["sstem_upsample_bilinear2x_f32"]
    per4 = torch.empty_like(product)
    _call(inst.lib, "sstem_upsample_bilinear2x_f32", _p(x), _p(per4), planes, H, W)
    monkeypatch.delenv("SSTEM_UPSAMPLE_TILED")
    _check(per4, ref, S, N_UP, "up-sampling forward, 4-per-thread", "%dx%dx%d (SSTEM_UPSAMPLE_TILED=0)" % (planes, H, W))
    assert torch.equal(per4, product), _which(planes, H, W)
    if _which(planes, H, W)[0] != "tiled":
        monkeypatch.setenv("SSTEM_UPSAMPLE_WIDE", "0")
        assert torch.equal(per4, _upsample(x))


# ---- up-sampling backward ---------------------------------------------------------------------------------------------------------------

def _which_bwd(planes, H, W):
    TW = 64 if W >= 64 else (32 if W >= 32 else 16)
    tiles = _ceil(W, TW) * _ceil(H, 256 // TW)
    gy = planes if tiles * planes <= 16384 else _ceil(16384, tiles)
    return "<%d,%d>" % (TW, 256 // TW), tiles, max(1, min(gy, 65535))


# (planes, H, W, template, tiles, grid y)
BACKWARD_CASES = [
    (3, 5, 7, "<16,16>", 1, 3),                   # odd W: the Python gate never sends one
    (2, 1, 1, "<16,16>", 1, 2),                   # one pixel gathers its 2 x 2 outputs (ry = rx = 0)
    (17000, 5, 7, "<16,16>", 1, 16384),           # 17000 > 16384: planes 0 .. 615 walk to plane + 16384
    (2, 9, 33, "<32,8>", 4, 2),                   # W = 32 + 1, H = 8 + 1: four tiles, three of them ragged
    (4200, 9, 33, "<32,8>", 4, 4096),             # 16800 > 16384: 4096 rows, planes 0 .. 103 walk
    (2, 5, 65, "<64,4>", 4, 2),                   # W = 64 + 1, H = 4 + 1
    (4200, 5, 65, "<64,4>", 4, 4096),
    (2, 130, 200, "<64,4>", 132, 2),              # 4 x 33 tiles: the fourth 8 columns wide, the 33rd 2 rows high
]


@pytest.mark.parametrize("planes,H,W,template,tiles,gy", BACKWARD_CASES)
def test_upsample_backward_every_element(planes, H, W, template, tiles, gy):
    assert _which_bwd(planes, H, W) == (template, tiles, gy)
    lib = sstem_native.load_library()
    g = torch.randn(planes, 2 * H, 2 * W, device="cuda", generator=_gen(2000 + planes + H + W))
    gin = torch.full((planes, H, W), float("nan"), device="cuda")
    _call(lib, "sstem_upsample_bilinear2x_backward_f32", _p(g), _p(gin), planes, H, W)
    ref, S = upsample2x_backward_ref64(g, H, W)
    _check(gin, ref, S, N_UP_BWD, "up-sampling backward, " + template, "%dx%dx%d" % (planes, H, W))
    again = torch.full((planes, H, W), float("nan"), device="cuda")
    _call(lib, "sstem_upsample_bilinear2x_backward_f32", _p(g), _p(again), planes, H, W)
    assert torch.equal(gin, again)


# ---- back-warp --------------------------------------------------------------------------------------------------------------------------

def _warp_flow(rng, B, H, W):
    """[B,2,H,W]: normal flows of sigma 4; a 40-pixel frame that points up to 60 pixels outside each border (both, in the corners);
    blocks of integer flows, of exact halves and of +-1e6."""
    flow = (rng.standard_normal((B, 2, H, W)) * 4).astype(np.float32)
    cols, rows = np.arange(W, dtype=np.float32)[None, None, :], np.arange(H, dtype=np.float32)[None, :, None]
    far = lambda: rng.uniform(0, 60, (B, H, W)).astype(np.float32)
    dx, dy = flow[:, 0], flow[:, 1]
    dx[:] = np.where(cols < 40, -cols - far(), np.where(cols >= W - 40, (W - 1 - cols) + far(), dx))
    dy[:] = np.where(rows < 40, -rows - far(), np.where(rows >= H - 40, (H - 1 - rows) + far(), dy))
    flow[:, :, 100:200, 100:300] = np.round(flow[:, :, 100:200, 100:300])
    flow[:, :, 300:400, 100:300] = np.round(flow[:, :, 300:400, 100:300]) + np.float32(0.5)
    flow[:, :, 500:600, 100:300] = np.where(rng.random((B, 2, 100, 200)) < 0.5, np.float32(-1e6), np.float32(1e6))
    assert np.isfinite(flow).all() and np.abs(flow).max() <= 1e9          # beyond that numpy's int64 cast is undefined
    return flow


@pytest.mark.parametrize("C", [1, 3])
def test_warp_every_element_equals_the_oracle_beyond_the_grid_wrap(C):
    """2 x 1030 x 1027 = 2 115 620 pixels against 8192 workgroups x 256 = 2 097 152 threads: the last 18 468 pixels, all inside the second
    image (p / plane = 1), are a thread's second trip.  The kernel adds four separately rounded products in stack order, as the reference
    module does, so its numpy restatement is reproduced bit for bit (a compiler that fused a product into the sum would show here)."""
    from oracle import warp_numpy
    from utils.image_warp_torch import SpatialTransformation
    B, H, W = 2, 1030, 1027
    assert B * H * W == 2115620 > 256 * 32 * 256 == 2097152 and 256 * 32 * 256 > H * W
    rng = np.random.default_rng(40 + C)
    img = rng.random((B, C, H, W), dtype=np.float32)
    flow = _warp_flow(rng, B, H, W)
    got = SpatialTransformation(use_gpu=True)(torch.from_numpy(img).cuda(), torch.from_numpy(flow).cuda().permute(0, 2, 3, 1)).cpu().numpy()
    want = warp_numpy.warp(img, flow)
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, (bad.shape[0], bad[:4].tolist())
    assert np.count_nonzero(want[:, :, 40:-40, 40:-40]) > 0.9 * want[:, :, 40:-40, 40:-40].size and (want[:, :, 500:600, 100:300] == 0).all()


# ---- Adam -------------------------------------------------------------------------------------------------------------------------------

ADAM_N = 3 * 524288 + 5                           # 2048 workgroups x 256 threads = 524 288: every thread makes three trips, five make four
ADAM_HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)


@pytest.fixture(scope="module")
def adam_state():
    state = adam_inputs(ADAM_N, _gen(77), device="cuda")
    yield state


def _adam_launch(state, wd, step):
    """One launch of sstem_adam_step_f32 on copies of (p, m, v); returns the new (p, m, v)."""
    lib = sstem_native.load_library()
    p, g, m, v = state
    p, m, v = p.clone(), m.clone(), v.clone()
    _call(lib, "sstem_adam_step_f32", _p(p), _p(g), _p(m), _p(v), ADAM_N, ADAM_HP["lr"], ADAM_HP["b1"], ADAM_HP["b2"], ADAM_HP["eps"], wd, step)
    return p, m, v


def _adam_check(new, state, wd, step, what):
    p1, m1, v1, S_p, S_m, S_v = adam_ref64(*state, wd=wd, step=step, **ADAM_HP)
    _check(new[1], m1, S_m, N_ADAM_M, "Adam, exp_avg", what)
    _check(new[2], v1, S_v, N_ADAM_V, "Adam, exp_avg_sq", what)
    _check(new[0], p1, S_p, N_ADAM_P, "Adam, parameter (of its composite S_p)", what)


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("step", [1, 2, 1000])
def test_adam_one_launch_every_element(adam_state, step, wd):
    assert 3 * (256 * 8) * 256 < ADAM_N < 4 * (256 * 8) * 256               # grid_1d caps the grid at 2048 workgroups
    new = _adam_launch(adam_state, wd, step)
    _adam_check(new, adam_state, wd, step, "step %d, wd %g" % (step, wd))


def test_adam_five_consecutive_steps_every_element(adam_state):
    """Five launches in a row, steps 1 .. 5, on one state; each is held to one reference step started from the kernel's own previous
    float32 state, so the bound stays the bound of one step."""
    lib = sstem_native.load_library()
    p, g, m, v = (t.clone() for t in adam_state)
    gen = _gen(78)
    for step in range(1, 6):
        before = (p.clone(), g, m.clone(), v.clone())
        _call(lib, "sstem_adam_step_f32", _p(p), _p(g), _p(m), _p(v), ADAM_N, ADAM_HP["lr"], ADAM_HP["b1"], ADAM_HP["b2"], ADAM_HP["eps"], 1e-2, step)
        _adam_check((p, m, v), before, 1e-2, step, "consecutive step %d" % step)
        del before
        g = g * (0.5 + torch.rand(ADAM_N, device="cuda", generator=gen))          # another gradient for the next step


# ---- 2 x 2 pooling ----------------------------------------------------------------------------------------------------------------------

def _pool_pair(kind, x):
    """Output and input gradient of hipnn.functional.pool_module and of the torch module on the same GPU tensors."""
    import hipnn.functional as HF
    m = torch.nn.MaxPool2d(2) if kind == "max" else torch.nn.AvgPool2d((2, 2), (2, 2))
    xa, xb = x.detach().requires_grad_(True), x.detach().clone().requires_grad_(True)
    ya, yb = HF.pool_module(m, xa), m(xb)
    g = torch.randn(yb.shape, device="cuda", generator=_gen(3100))
    ya.backward(g)
    yb.backward(g)
    torch.cuda.synchronize()
    return ya.detach(), yb.detach(), xa.grad, xb.grad


def _pool_input(shape, seed, offset=0):
    n = int(np.prod(shape))
    store = torch.relu(torch.randn(n + offset, device="cuda", generator=_gen(seed)))          # many exact ties at zero
    x = store[offset:].view(shape)
    x[0, 0, 0, 1] = float("nan")
    return x


@pytest.mark.parametrize("kind", ["max", "avg"])
@pytest.mark.parametrize("shape,kernel", [
    ((1, 17, 1000, 1000), "vector"),          # 17 * 500 * 500 = 4 250 000 outputs > 16384 * 256 = 4 194 304: the forward wraps once, the backward
                                              # (17 000 000 inputs) four times
    ((1, 17, 1001, 1002), "vector"),          # odd H: the last row has no window and a zero gradient
    ((1, 17, 1000, 1001), "scalar"),          # odd W: rows are not 8-byte aligned, the scalar kernel; the last column has no window
])
def test_pool2x2_beyond_the_grid_wrap_bit_for_bit(shape, kernel, kind):
    N, C, H, W = shape
    assert N * C * (H // 2) * (W // 2) > 256 * 64 * 256 and N * C * H * W > 4 * 256 * 64 * 256
    x = _pool_input(shape, 3000 + W)
    assert (kernel == "vector") == (W % 2 == 0 and x.data_ptr() % 8 == 0)
    ya, yb, ga, gb = _pool_pair(kind, x)
    assert ya.shape == yb.shape and torch.equal(torch.nan_to_num(ya, nan=-7.0), torch.nan_to_num(yb, nan=-7.0))
    assert torch.equal(torch.nan_to_num(ga, nan=-7.0), torch.nan_to_num(gb, nan=-7.0))


@pytest.mark.parametrize("kind", ["max", "avg"])
def test_pool2x2_pointer_gate_sends_a_4_byte_aligned_plane_to_the_scalar_kernel(kind):
    """[2,3,8,10] as a contiguous view that starts one float into its storage: W is even but (in & 7) = 4, so the launcher's own gate takes the
    scalar kernel (the vector kernel's 8-byte row reads would be misaligned).  The only alignment case: every other pointer here is as
    aligned as its header requires."""
    x = _pool_input((2, 3, 8, 10), 3200, offset=1)
    assert x.is_contiguous() and x.data_ptr() % 8 == 4 and x.shape[3] % 2 == 0
    ya, yb, ga, gb = _pool_pair(kind, x)
    assert torch.equal(torch.nan_to_num(ya, nan=-7.0), torch.nan_to_num(yb, nan=-7.0))
    assert torch.equal(torch.nan_to_num(ga, nan=-7.0), torch.nan_to_num(gb, nan=-7.0))
    aligned = x.clone()
    assert aligned.data_ptr() % 8 == 0
    assert torch.equal(torch.nan_to_num(_pool_pair(kind, aligned)[0], nan=-7.0), torch.nan_to_num(ya, nan=-7.0))      # vector == scalar


# ---- uint8 edge -------------------------------------------------------------------------------------------------------------------------

U8_NPIX = 2048 * 256 + 77                         # 2048 workgroups x 256 threads = 524 288: 77 threads make a second trip


@pytest.mark.parametrize("replicas", [1, 3])
def test_gray_u8_to_f32_beyond_the_grid_wrap_bit_for_bit(replicas):
    lib = sstem_native.load_library()
    img = torch.randint(0, 256, (U8_NPIX,), device="cuda", generator=_gen(4000), dtype=torch.int64).to(torch.uint8)
    img[:256] = torch.arange(256, device="cuda").to(torch.uint8)
    img[-256:] = torch.arange(256, device="cuda").to(torch.uint8).flip(0)        # every byte value on the second trip too
    out = torch.full((replicas, U8_NPIX), float("nan"), device="cuda")
    _call(lib, "sstem_gray_u8_to_f32", _p(img), _p(out), U8_NPIX, replicas)
    table = (torch.arange(256, dtype=torch.float32) / torch.tensor(255.0)).cuda()          # float32(k) / float32(255), divided on the host
    assert table[255].item() == 1.0 and table[0].item() == 0.0
    want = table[img.long()]
    for r in range(replicas):
        assert torch.equal(out[r], want), r


@pytest.mark.parametrize("clamp01", [0, 1])
def test_f32_to_gray_u8_rule_at_its_edges_and_beyond_the_grid_wrap(clamp01):
    lib = sstem_native.load_library()
    f = np.float32
    n256, m1 = f(256.0) / f(255.0), f(-1.0) / f(255.0)
    sown = np.array([-1.0, -0.999, -0.0, n256, np.nextafter(n256, f(0)), np.nextafter(n256, f(2)), m1, np.nextafter(m1, f(0)),
                     np.nextafter(m1, f(-1)), 1.0, 2.0, 1e10, -1e10, 4e16, 3.5e16, 1e19, -1e19, np.inf, -np.inf, np.nan], f)
    v = torch.rand(U8_NPIX, device="cuda", generator=_gen(4100)) * 1.5 - 0.2                # uniform in [-0.2, 1.3]
    s = torch.from_numpy(sown).cuda()
    v[:s.numel()] = s
    v[-s.numel():] = s                                                                      # on the second trip too
    v[1000:1000 + s.numel()] = -s
    out = torch.full((U8_NPIX,), 99, device="cuda", dtype=torch.uint8)
    _call(lib, "sstem_f32_to_gray_u8", _p(v), _p(out), U8_NPIX, clamp01)
    want = f32_to_u8_ref(v, clamp01)
    bad = torch.nonzero(out != want)
    assert bad.numel() == 0, (bad.numel(), [(int(i), float(v[i]), int(out[i]), int(want[i])) for i in bad[:6, 0]])
    if not clamp01:                                               # the rule's own examples, by the scaled value
        scaled = (v * 255.0)
        assert (out[scaled == 256.0] == 0).all() and (scaled == 256.0).any()
        assert (out[scaled == -1.0] == 255).all() and (scaled == -1.0).any()
        assert (out[~torch.isfinite(v) | (v.abs() >= 1e19)] == 0).all()
