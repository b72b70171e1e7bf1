"""The fold synthesis contract of include/sstem_fold.h, restated in numpy: gen_flow, the byte image_warp and the fused training sample,
vectorised but with the contract's operation order (every multiply and add its own rounding, in float64 for the flow and float32 for
the warp), so its results are comparable bit for bit with the reference's fixture (tests/golden/fold.npz) and with the kernels.

It is the project's own statement of the arithmetic, not the reference's code: it works per pixel from the fold's row of doubles
(``scalars``), on any window of a plane, and ``variant`` switches in the deliberate mistakes that tests/test_fold_cpu.py shows the
fixture to catch.  The images of the fixture and of the GPU tests come from the seeded recipe ``image`` and are not stored."""
import math
import random

import numpy as np

PARAMS = 10
MINA = 0.000000001

# variants of the arithmetic that the fixture must tell from the contract
MUTANTS = ("fused_multiply", "lt_for_le", "simplified_sign", "clamped_weights", "rounded_bytes")


def gen_line(p1, p2):
    """k, b of the line through two [row, column] points (the reference's convention: a zero denominator becomes 1e-9)."""
    den = p2[1] - p1[1]
    if den == 0:
        den = MINA
    k = (p2[0] - p1[0]) / den
    return k, p1[0] - (k * p1[1])


def scalars(k, b, line_width=5, fold_width=10, dis_k=0.1):
    """The fold's row of doubles (include/sstem_fold.h), derived as the contract says: Python float arithmetic and the math module."""
    norm = math.sqrt(k ** 2 + 1)
    ndk = -dis_k
    dis_b = (fold_width - line_width) - ndk * line_width
    angle = math.atan(1 / MINA if k == 0 else 1 / k)
    return np.array([k, b, norm, line_width, fold_width, ndk, dis_b, math.cos(angle), math.sin(angle), 1.0 if k > 0 else 0.0],
                    dtype=np.float64)


def image(seed, H, W, C=None):
    """The seeded uint8 test image: no zero pixel (so a black pixel of a degraded image comes from the fold), every other byte."""
    shape = (H, W) if C is None else (H, W, C)
    return np.random.default_rng(seed).integers(1, 256, size=shape, dtype=np.uint8)


def _fma64(a, b, c):
    """round(a * b + c) with one rounding, through the 64-bit mantissa of the x87 long double (exact for the small integers here)."""
    return (np.asarray(a, np.longdouble) * np.asarray(b, np.longdouble) + np.asarray(c, np.longdouble)).astype(np.float64)


def flow(row, H, W, window=None, variant=None):
    """flow, flow2 [h,w,2] float32 and mask [h,w] uint8 on the window (off_y, off_x, h, w) of an H x W plane (default: the plane)."""
    k, b, norm, lw, fw, ndk, dis_b, cos_p, sin_p, k_pos = (float(v) for v in row)
    oy, ox, h, w = window if window is not None else (0, 0, H, W)
    x = np.broadcast_to(np.arange(ox, ox + w, dtype=np.float64)[None, :], (h, w))
    y = np.broadcast_to(np.arange(oy, oy + h, dtype=np.float64)[:, None], (h, w))
    if variant == "fused_multiply":
        d = (_fma64(k, x, -y) + b) / norm
    else:
        d = (((k * x) - y) + b) / norm
    sign = np.where(d > 0, 1.0, np.where(d < 0, -1.0, 0.0))
    a = np.abs(d)
    if variant == "lt_for_le":
        mask = np.where(a < lw, 0, 1).astype(np.uint8)
    else:
        mask = np.where(a <= lw, 0, 1).astype(np.uint8)
    m1 = np.where(a < lw, 0.0, 1.0)
    m2 = np.where(a < fw, 0.0, 1.0)
    s = _fma64(ndk, a, dis_b) if variant == "fused_multiply" else ndk * a + dis_b
    s = np.where(s < 0, 0.0, s)
    s1 = s * m1 + a * (1.0 - m1)
    s2 = s * m2 + a * (1.0 - m2)
    if variant == "simplified_sign":                   # selects instead of the products by the sign: no -0.0 where d == 0
        dis = np.where(d > 0, s1, np.where(d < 0, -s1, 0.0))
        dis2 = np.where(d > 0, -s2, np.where(d < 0, s2, 0.0))
    else:
        dis = s1 * sign
        dis2 = s2 * (-sign)
    out = []
    for v in (dis, dis2):
        c, n = v * cos_p, v * sin_p
        f = np.empty((h, w, 2), dtype=np.float32)
        if k_pos != 0.0:
            f[..., 0], f[..., 1] = c, -n
        else:
            f[..., 0], f[..., 1] = -c, n
        out.append(f)
    return out[0], out[1], mask


def warp(im, fl, mode="bilinear", window=None, variant=None):
    """image_warp of the uint8 plane im [H,W] or [H,W,C] by fl (float32 [h,w,2], given on the window) -> uint8 [h,w(,C)]."""
    H, W = im.shape[:2]
    oy, ox, h, w = window if window is not None else (0, 0, H, W)
    assert fl.shape == (h, w, 2) and fl.dtype == np.float32 and im.dtype == np.uint8
    col = np.arange(ox, ox + w, dtype=np.int64)[None, :]
    rw = np.arange(oy, oy + h, dtype=np.int64)[:, None]
    fl_floor = np.floor(fl)
    x0u = col + fl_floor[..., 0].astype(np.int32)
    y0u = rw + fl_floor[..., 1].astype(np.int32)
    x0, y0 = np.clip(x0u, 0, W - 1), np.clip(y0u, 0, H - 1)
    if mode == "nearest":
        return im[y0, x0]
    assert mode == "bilinear"
    x1, y1 = np.clip(x0 + 1, 0, W - 1), np.clip(y0 + 1, 0, H - 1)
    one = np.float32(1)
    if variant == "clamped_weights":                   # the fraction measured from the clamped corner
        xw = ((col + fl[..., 0]) - x0).astype(np.float32)
        yw = ((rw + fl[..., 1]) - y0).astype(np.float32)
    else:
        xw, yw = fl[..., 0] - fl_floor[..., 0], fl[..., 1] - fl_floor[..., 1]
    wa, wb, wc, wd = (one - xw) * (one - yw), (one - xw) * yw, xw * (one - yw), xw * yw
    if im.ndim == 3:
        wa, wb, wc, wd = wa[..., None], wb[..., None], wc[..., None], wd[..., None]
    f32 = np.float32
    v = ((wa * im[y0, x0].astype(f32) + wb * im[y1, x0].astype(f32)) + wc * im[y0, x1].astype(f32)) + wd * im[y1, x1].astype(f32)
    assert v.dtype == np.float32
    if variant == "rounded_bytes":
        return np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return v.astype(np.int64).astype(np.uint8)          # truncation; the sum is in [0, 256)


def degrade(clean, interp, row, window, gt_line=False, variant=None):
    """The fused sample on a window of the plane: dict of deformed (uint8 [h,w]), flow2 ([2,h,w] float32), im ([6,h,w] float32),
    lb ([1,h,w] float32) and zero_count."""
    H, W = clean.shape
    oy, ox, h, w = window
    fl, fl2, mask = flow(row, H, W, window, variant)
    deformed = warp(clean, fl, "bilinear", window, variant) * mask
    f255 = np.float32(255)
    dv = deformed.astype(np.float32) / f255
    out = {"deformed": deformed, "flow2": np.ascontiguousarray(np.transpose(fl2, (2, 0, 1))), "zero_count": int((deformed == 0).sum())}
    if interp is not None:
        iv = interp[oy:oy + h, ox:ox + w].astype(np.float32) / f255
        out["im"] = np.stack([dv, dv, dv, iv, iv, iv])
    lb = clean[oy:oy + h, ox:ox + w].astype(np.float32) / f255
    if gt_line:
        lb = np.where(deformed == 0, np.float32(0), lb)
    out["lb"] = lb[None]
    return out


def draw_fold(rng, height, width):
    """One candidate fold from a random.Random, value by value as the contract of data/fold_degradation.draw_fold states it:
    randint(5, 20), randint(line_width + 1, 80), two distinct borders of 1..4, a point on each, uniform(0.00001, 0.1)."""
    line_width = rng.randint(5, 20)
    fold_width = rng.randint(line_width + 1, 80)
    k1 = rng.randint(1, 4)
    k2 = rng.randint(1, 4)
    while k1 == k2:
        k2 = rng.randint(1, 4)
    pts = []
    for side in (k1, k2):
        if side == 1:
            pts.append([0, rng.randint(1, width - 1)])
        elif side == 2:
            pts.append([rng.randint(1, height - 1), width])
        elif side == 3:
            pts.append([height, rng.randint(1, width - 1)])
        else:
            pts.append([rng.randint(1, height - 1), 0])
    dis_k = rng.uniform(0.00001, 0.1)
    k, b = gen_line(pts[0], pts[1])
    return k, b, line_width, fold_width, dis_k


# ---- the fixture's cases -------------------------------------------------------------------------------------------------------------
# (a) name -> (H, W, k, b, line_width, fold_width, dis_k, image seed)
FOLD_CASES = {
    "k0_ties":      (40, 56, 0.0, 17.0, 5, 10, 0.05, 1),                       # k == 0, integer b: a == line_width, a == fold_width, d == 0 rows
    "k0_lw20":      (40, 56, 0.0, 20.0, 20, 21, 0.1, 2),                       # dis_abs == line_width on the top row, fold_width = line_width + 1
    "k_plus1":      (40, 56, 1.0, -3.0, 5, 10, 0.1, 3),
    "k_minus1":     (40, 56, -1.0, 40.0, 6, 13, 0.02, 4),
    "zero_den":     (40, 56) + gen_line([0, 10], [40, 10]) + (5, 10, 0.1, 5),  # a vertical line: k = 40 / 1e-9
    "fw_lw_plus1":  (40, 56, 0.37, 9.25, 7, 8, 0.07, 6),
    "wide_20_80":   (40, 56, -0.6, 35.0, 20, 80, 0.1, 7),
    "non_square":   (33, 61) + gen_line([0, 13], [33, 47]) + (5, 12, 0.031, 8),
    "tiny_dis_k":   (40, 56) + gen_line([21, 56], [40, 3]) + (9, 30, 0.00001, 9),
    "steep":        (40, 56, 7.5, -150.0, 5, 10, 0.1, 10),
    "third":        (40, 56, 1 / 3, 0.0, 5, 10, 0.1, 11),                      # k * x rounds to the integer y: d == 0 where a fused k * x - y is not
    "shallow_neg":  (48, 64, -0.015625, 24.0, 12, 40, 0.09, 12),
}

# (b) seeds of random.seed for the reference's rejection loop, on a DEGRADE_SIZE plane with a DEGRADE_OFFSET border
DEGRADE_SIZE, DEGRADE_OFFSET, DEGRADE_MIN_ZERO = 64, 8, 100
DEGRADE_SEEDS = (0, 3, 10, 15, 31)                       # 10, 15 and 31 reject their first candidate
DEGRADE_IMAGE_SEED = 100


def fold_case(name):
    H, W, k, b, lw, fw, dis_k, seed = FOLD_CASES[name]
    return H, W, (k, b, lw, fw, dis_k), image(seed, H, W)


def rejection_loop(clean, seed, size=DEGRADE_SIZE, offset=DEGRADE_OFFSET, min_zero=DEGRADE_MIN_ZERO):
    """The reference's loop restated on fold_ref: draw, degrade the centre window, redraw below min_zero black pixels.
    Returns (deformed, flow2 [2,h,w], candidates drawn, the accepted fold)."""
    rng = random.Random(seed)
    window = (offset, offset, size - 2 * offset, size - 2 * offset)
    drawn = 0
    while True:
        fold = draw_fold(rng, size, size)
        drawn += 1
        got = degrade(clean, None, scalars(*fold), window)
        if got["zero_count"] >= min_zero:
            return got["deformed"], got["flow2"], drawn, fold
