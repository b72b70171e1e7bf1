"""The contracts of include/sstem_display.h, restated in numpy.

``flow_to_image`` is the colour code of a flow field: the reference's utils/flow_display.py as it runs under NumPy 2 (float32 up to the
maximum radius, float64 from the division on), operation by operation, with two additions the tests need: ``ulps`` moves the arctan2
result by that many float64 steps (clamped to +-np.pi), which is the one operation whose bits a device cannot promise, and ``mutant``
names one deliberate mistake that tests/test_flow_color_cpu.py shows the fixture (tests/golden/flow_color.npz) to catch.
``sff_outputs`` is the image tail of the inference scripts, which has no transcendental and is held bit for bit.

The cases of the fixture and of the GPU tests come from ``cases()``: seeded, the same arrays everywhere."""
import numpy as np

H0, W0 = 67, 130                     # every case unless said
ATAN2_ULPS = 4                       # k: see DESIGN 4l -- the two libraries' atan2 bounds for double, summed, plus one
AMBIGUOUS_CAP = 1.0e-3               # a condition on the inputs: the share of bytes that k steps of the angle can move
EPS = np.finfo(float).eps            # 2^-52, a float64 scalar

MUTANTS = ("batch_max", "maxrad_f64", "no_eps", "nan_maxrad", "k1_not_wrapped", "no_075")


def make_wheel():
    """The 55 colours, uint8 [55,3]: six arcs, on each one channel ramps by floor(255 i / n) while the others hold 0 or 255."""
    arcs = ((15, (255, None, 0), +1), (6, (None, 255, 0), -1), (4, (0, 255, None), +1), (11, (0, None, 255), -1),
            (13, (None, 0, 255), +1), (6, (255, 0, None), -1))
    rows = []
    for n, pattern, direction in arcs:
        for i in range(n):
            ramp = (255 * i) // n
            rows.append([(ramp if direction > 0 else 255 - ramp) if c is None else c for c in pattern])
    return np.array(rows, dtype=np.uint8)


WHEEL = make_wheel()


def shift_ulps(x, n):
    """x (float64) moved n representable steps up (n > 0) or down, then clamped to [-pi, pi]."""
    for _ in range(abs(int(n))):
        x = np.nextafter(x, np.inf if n > 0 else -np.inf)
    return np.clip(x, -np.pi, np.pi)


def max_radius(flow, mutant=None):
    """maxrad of one [H,W,2] float32 image: a float32 scalar, or -1 (a Python int, as in the reference)."""
    u, v = flow[..., 0].copy(), flow[..., 1].copy()
    unknown = (np.abs(u) > 1e7) | (np.abs(v) > 1e7)
    u[unknown] = 0
    v[unknown] = 0
    if mutant == "maxrad_f64":
        rad = np.sqrt(u.astype(np.float64) ** 2 + v.astype(np.float64) ** 2)
    else:
        rad = np.sqrt(u * u + v * v)
        assert rad.dtype == np.float32
    m = np.max(rad)
    if mutant == "nan_maxrad":
        return m
    return m if m > -1 else -1                    # max(-1, nan) keeps -1


def flow_to_image(flow, ulps=0, mutant=None, maxrad=None):
    """[H,W,2] float32 -> [H,W,3] uint8.  Never writes ``flow`` (the reference zeroes unknown pixels in place)."""
    flow = np.asarray(flow)
    assert flow.dtype == np.float32 and flow.ndim == 3 and flow.shape[2] == 2
    u, v = flow[..., 0].copy(), flow[..., 1].copy()
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        unknown = (np.abs(u) > 1e7) | (np.abs(v) > 1e7)
        u[unknown] = 0
        v[unknown] = 0
        if maxrad is None:
            maxrad = max_radius(flow, mutant)
        d = np.float64(maxrad) + (0.0 if mutant == "no_eps" else EPS)
        u = u.astype(np.float64) / d
        v = v.astype(np.float64) / d
        nan = np.isnan(u) | np.isnan(v)
        u[nan] = 0
        v[nan] = 0
        rad = np.sqrt(u * u + v * v)
        a = shift_ulps(np.arctan2(-v, -u), ulps) / np.pi
        fk = (a + 1) / 2 * (len(WHEEL) - 1) + 1
        k0 = np.floor(fk).astype(int)
        k1 = k0 + 1
        if mutant != "k1_not_wrapped":
            k1[k1 == len(WHEEL) + 1] = 1
        f = fk - k0
        img = np.zeros(u.shape + (3,), dtype=np.uint8)
        for c in range(3):
            tmp = WHEEL[:, c].astype(np.float64)
            col = (1 - f) * (tmp[k0 - 1] / 255) + f * (tmp[k1 - 1] / 255)
            near = rad <= 1
            col[near] = 1 - rad[near] * (1 - col[near])
            if mutant != "no_075":
                col[~near] *= 0.75
            img[..., c] = np.floor(255 * col * (1 - nan)).astype(np.uint8)
        img[unknown] = 0
    return img


def flow_color_batch(flow_b2hw, ulps=0, mutant=None):
    """[B,2,H,W] float32 -> [B,H,W,3] uint8, every image by its own maximum."""
    hwc = np.ascontiguousarray(np.transpose(flow_b2hw, (0, 2, 3, 1)))
    shared = None
    if mutant == "batch_max":
        rads = [max_radius(im) for im in hwc]
        shared = max(rads, key=lambda r: -1.0 if r != r else float(r))
    return np.stack([flow_to_image(im, ulps, None if mutant == "batch_max" else mutant, shared) for im in hwc])


def byte_range(flow_hw2, k=ATAN2_ULPS):
    """(lo, hi, step0) uint8 [H,W,3]: the minimum and the maximum of the restatement over the 2k + 1 angle steps, and step 0 itself."""
    steps = np.stack([flow_to_image(flow_hw2, n) for n in range(-k, k + 1)])
    return steps.min(0), steps.max(0), steps[k]


# ---- the image tail ------------------------------------------------------------------------------------------------------------------
def to_u8(x):
    """(x * 255).astype(np.uint8) on float32 as numpy does it on x86-64: truncation to a wide integer, the low 8 bits; NaN and
    |v| >= 2^63 give 0 (stated with integers, so it does not depend on the host's cast)."""
    v = np.asarray(x, dtype=np.float32) * np.float32(255)
    ok = np.isfinite(v) & (np.abs(v) < 9.0e18)
    w = np.where(ok, v, 0).astype(np.float64)                 # float32 -> float64 is exact
    return (np.trunc(w).astype(np.int64) & 0xFF).astype(np.uint8)


def luminance(rgb):
    """PIL's convert('L') on uint8 [...,3]."""
    r, g, b = (rgb[..., c].astype(np.int64) for c in range(3))
    return ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16).astype(np.uint8)


def sff_outputs(pred, warped, interp):
    """pred [B,H,W], warped [B,3,H,W] float32, interp [B,H,W] uint8 -> (pred_u8 [B,H,W], warped_rgb [B,H,W,3], stitch [B,H,W])."""
    rgb = np.ascontiguousarray(np.transpose(to_u8(warped), (0, 2, 3, 1)))
    L = luminance(rgb)
    return to_u8(pred), rgb, np.where(L < 2, interp, L).astype(np.uint8)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def _smooth(H, W):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    u = 3.0 * np.sin(x / 17.0) + 0.05 * (y - H / 2)
    v = 2.0 * np.cos(y / 11.0) - 0.03 * (x - W / 3)
    return np.stack([u, v], -1).astype(np.float32)


def cases():
    """name -> [H,W,2] float32 (single images) in a fixed order."""
    rng = np.random.default_rng(20261020)
    H, W = H0, W0
    out = {}
    out["smooth"] = _smooth(H, W)
    out["smooth_noise"] = (_smooth(H, W) + 0.3 * rng.standard_normal((H, W, 2))).astype(np.float32)
    out["randn30"] = (30.0 * rng.standard_normal((H, W, 2))).astype(np.float32)
    out["tiny"] = (1e-20 * rng.standard_normal((H, W, 2))).astype(np.float32)
    out["zeros"] = np.zeros((H, W, 2), dtype=np.float32)
    knots = (2.0 * rng.standard_normal((H, W, 2))).astype(np.float32)
    knots[3, :, 1] = 0.0                                                     # rows with v = 0, either sign of zero
    knots[40, :, 1] = -0.0
    knots[:, 5, 0] = 0.0                                                     # columns with u = 0
    knots[:, 99, 0] = -0.0
    knots[20, 20] = (0.0, 0.0)
    knots[21, 21] = (-0.0, -0.0)
    knots[22, 22] = (1.5, -0.0)                                              # atan2(+0, -1.5) = pi: k0 = 55, k1 wraps
    out["knots"] = knots
    out["integers"] = rng.integers(-20, 21, size=(H, W, 2)).astype(np.float32)
    unknown = (4.0 * rng.standard_normal((H, W, 2))).astype(np.float32)
    unknown[10, 11, 0] = 2e7
    unknown[50, 100, 1] = -np.inf
    out["unknown"] = unknown
    one_nan = (0.8 * rng.standard_normal((H, W, 2))).astype(np.float32)
    one_nan[33, 64, 0] = np.nan
    out["one_nan"] = one_nan
    out["all_nan"] = np.full((H, W, 2), np.nan, dtype=np.float32)
    out["1x1"] = np.array([[[0.25, -3.0]]], dtype=np.float32)
    out["1x131"] = (5.0 * rng.standard_normal((1, 131, 2))).astype(np.float32)
    out["131x1"] = (5.0 * rng.standard_normal((131, 1, 2))).astype(np.float32)
    return out


def batch_case():
    """[4,2,H,W] float32: maxima of 1e-3, 5 and 4e6, and a fourth image holding a NaN -- a maximum shared across the batch, or a NaN flag
    that leaks into a neighbour, changes every byte of some image."""
    rng = np.random.default_rng(4)
    base = rng.standard_normal((4, 2, H0, W0))
    base /= np.sqrt((base ** 2).sum(1)).max(axis=(1, 2))[:, None, None, None]      # every image's largest radius is 1
    flow = (base * np.array([1e-3, 5.0, 4e6, 2.0])[:, None, None, None]).astype(np.float32)
    flow[3, 1, 7, 9] = np.nan
    return flow


def tiled(flow_hw2, H, W):
    """([H,W,2] float32, index [H*W]): the pixels of a small image repeated in order until they fill H x W.  Every pixel of the small
    image occurs, so the maximum radius is the small image's and pixel i of the large one has the bytes of pixel index[i] of the small
    one: a reference for a million pixels at the price of a few thousand."""
    small = flow_hw2.reshape(-1, 2)
    assert H * W >= len(small)
    index = np.arange(H * W) % len(small)
    return np.ascontiguousarray(small[index].reshape(H, W, 2)), index


def gather_range(rng_small, index, H, W):
    """byte_range of the small image -> the same of its tiled image."""
    return tuple(a.reshape(-1, 3)[index].reshape(H, W, 3) for a in rng_small)


def grid_cap_case(cap_pixels, base="smooth_noise"):
    """(flow, index, base): 1025 x 1025 tiled from a 67 x 130 case, which passes ``cap_pixels`` = 4096 workgroups of 256 by a ragged
    remainder; the tile's length shares no factor pattern with the stride, so a lane that walked wrongly would land on other bytes."""
    H = W = 1025
    assert cap_pixels < H * W < 2 * cap_pixels and (H * W - cap_pixels) % 256 != 0 and cap_pixels % (H0 * W0) != 0
    flow, index = tiled(cases()[base], H, W)
    return flow, index, base


def gray_triples():
    """uint8 [n,3] for the luminance record: all 256 grey triples, extremes and seeded random triples."""
    rng = np.random.default_rng(12)
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    ext = np.array([[r, g, b] for r in (0, 1, 2, 255) for g in (0, 1, 2, 255) for b in (0, 1, 2, 255)], dtype=np.uint8)
    return np.concatenate([grey, ext, rng.integers(0, 256, size=(400, 3), dtype=np.uint8)])
