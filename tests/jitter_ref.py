"""The colour-jitter contract of include/sstem_jitter.h, restated in numpy: PIL's byte blend in float32 with every product and sum its
own rounding, the chain of steps as one 256-entry table per sample with the contrast mean taken through the histogram of the plane as
given, and the fold degradation that reads its section through such a table (composed with tests/fold_ref.py).

It is the project's own statement of the arithmetic, not PIL's code; ``variant`` switches in the deliberate mistakes that
tests/test_jitter_cpu.py shows the fixture (tests/golden/jitter.npz) to catch.  The images of the fixture and of the GPU tests come from
the seeded recipes below and are not stored."""
import numpy as np

import fold_ref as R

OPS = 4
NONE, BRIGHTNESS, CONTRAST, SATURATION = 0, 1, 2, 3

# variants of the arithmetic that the fixture must tell from the contract
MUTANTS = ("fused_multiply", "double_factor", "rounded_bytes", "mean_truncated", "mean_of_original", "reversed_order")


def blend(d, v, factor, variant=None):
    """Blend.c on bytes: v (integer array) towards the degenerate d by `factor` -> integer array in [0, 255]."""
    alpha = np.float32(factor)
    diff = (np.asarray(v, dtype=np.int64) - int(d)).astype(np.float32)
    if variant == "fused_multiply":                        # one rounding: the product is exact in double, and so is the sum here
        t = (np.float64(d) + np.float64(alpha) * diff.astype(np.float64)).astype(np.float32)
    elif variant == "double_factor":                       # the factor never narrowed, the arithmetic in double
        t = np.float64(d) + np.float64(factor) * diff.astype(np.float64)
    else:
        t = np.float32(d) + alpha * diff
        assert t.dtype == np.float32
    finite = np.isfinite(t)
    whole = np.where(finite, np.rint(t) if variant == "rounded_bytes" else np.trunc(t), 0).astype(np.int64)
    if 0 <= alpha <= 1:
        return whole & 0xFF
    return np.where(finite, np.where(t <= 0, 0, np.where(t >= 255, 255, whole)), 0)      # outside the contract: not finite stores 0


def mean_byte(hist, count, values, variant=None):
    """int(mean + 0.5) of the image whose bytes v became values[v]: (2 sum + count) // (2 count) in exact integers."""
    total = sum(int(h) * int(c) for h, c in zip(hist, values))
    if variant == "mean_truncated":
        return total // count
    return (2 * total + count) // (2 * count)


def table(hist, count, steps, variant=None):
    """The sample's table uint8 [256] from the histogram of its plane and its steps [(code, factor), ...], applied left to right."""
    assert len(steps) <= OPS
    cur = np.arange(256, dtype=np.int64)
    for code, factor in (reversed(steps) if variant == "reversed_order" else steps):
        if code == BRIGHTNESS:
            cur = blend(0, cur, factor, variant)
        elif code == CONTRAST:
            seen = np.arange(256) if variant == "mean_of_original" else cur
            cur = blend(mean_byte(hist, count, seen, variant), cur, factor, variant)
        else:
            assert code in (NONE, SATURATION), code
    return cur.astype(np.uint8)


def lut_of(plane, steps, variant=None):
    assert plane.dtype == np.uint8
    return table(np.bincount(plane.reshape(-1), minlength=256), plane.size, steps, variant)


def apply(plane, steps, variant=None):
    """The jittered plane: every byte through the plane's table."""
    return lut_of(plane, steps, variant)[plane]


def step_arrays(steps):
    """Per-sample step lists -> codes int32 [n, OPS], factors float32 [n, OPS], padded with (NONE, 0)."""
    codes, factors = np.zeros((len(steps), OPS), np.int32), np.zeros((len(steps), OPS), np.float32)
    for i, sample in enumerate(steps):
        for q, (code, factor) in enumerate(sample):
            codes[i, q], factors[i, q] = code, factor
    return codes, factors


def degrade(clean, interp, row, window, lut, gt_line=False):
    """fold_ref.degrade with the section read through `lut` (uint8 [256]): everything follows the jittered section except lb, which is
    the un-jittered window (zero on the jittered sample's black pixels with gt_line)."""
    out = R.degrade(lut[clean], interp, row, window, gt_line)
    oy, ox, h, w = window
    lb = clean[oy:oy + h, ox:ox + w].astype(np.float32) / np.float32(255)
    if gt_line:
        lb = np.where(out["deformed"] == 0, np.float32(0), lb)
    out["lb"] = lb[None]
    return out


def draw_jitter(rng, brightness, contrast, saturation):
    """The draws of data/color_jitter.draw_jitter, value by value: per nonzero strength one uniform(max(0, 1 - x), 1 + x) in the order
    brightness, contrast, saturation, then one shuffle of the list."""
    steps = []
    if brightness > 0:
        steps.append((BRIGHTNESS, rng.uniform(max(0, 1 - brightness), 1 + brightness)))
    if contrast > 0:
        steps.append((CONTRAST, rng.uniform(max(0, 1 - contrast), 1 + contrast)))
    if saturation > 0:
        steps.append((SATURATION, rng.uniform(max(0, 1 - saturation), 1 + saturation)))
    rng.shuffle(steps)
    return steps


# ---- the fixture's cases (tests/golden/make_jitter_golden.py) ------------------------------------------------------------------------
# (a) Image.blend(constant d, ramp, f) for every d: 0.6 and 1.1 tell a fused multiply-add and a double factor from float32, 1.3 a double
# factor, 1.0000001 the extrapolation branch next to 1
BLEND_FACTORS = (0.0, 0.5, 0.6, 1.0, 1.1, 1.3, 1.5, 1.0000001)

# (b) ImageEnhance chains: the six orders of (brightness, contrast, saturation), then two with a repeated enhancement
B_, C_, S_ = BRIGHTNESS, CONTRAST, SATURATION
CHAINS = (
    ((B_, 0.6), (C_, 1.1), (S_, 1.3)),
    ((B_, 1.1), (S_, 0.7), (C_, 0.6)),
    ((C_, 1.3), (B_, 0.6), (S_, 1.2)),
    ((C_, 0.6), (S_, 1.5), (B_, 1.3)),
    ((S_, 0.5), (B_, 1.1), (C_, 1.3)),
    ((S_, 1.1), (C_, 0.6), (B_, 1.1)),
    ((C_, 1.3), (C_, 0.6), (B_, 0.9)),
    ((B_, 1.3), (B_, 0.6), (C_, 1.1), (C_, 1.4)),
)


def _two_valued(H, W, low, n_high):
    a = np.full(H * W, low, dtype=np.uint8)
    a[:n_high] = low + 1
    return np.random.default_rng(H * W).permutation(a).reshape(H, W)


def images():
    """name -> uint8 image, in the fixture's order."""
    rng = np.random.default_rng(900)
    out = {
        "one": np.array([[137]], dtype=np.uint8),
        "zeros": np.zeros((5, 7), dtype=np.uint8),
        "full": np.full((5, 7), 255, dtype=np.uint8),
        "half": _two_valued(4, 6, 100, 12),                # mean 100.5 exactly: the degenerate is 101
        "below_half": _two_valued(37, 53, 100, 980),       # 1961 pixels, mean 100 + 980 / 1961: the degenerate is 100
        "noise": rng.integers(0, 256, size=(37, 53), dtype=np.uint8),
        "em": np.clip(np.rint(rng.normal(128.0, 12.0, size=(64, 64))), 0, 255).astype(np.uint8),      # a narrow histogram
    }
    return out


# (c) the fusion provider with color_jitter on, at the sizes of crop_ref's fusion cases
PROVIDER_SEEDS = (1, 2)
PROVIDER_JITTER = (0.5, 0.5, 0.5)
