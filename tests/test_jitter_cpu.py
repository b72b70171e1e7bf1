"""Colour jitter without a GPU: the numpy restatement of the contract (tests/jitter_ref.py) against PIL's recorded bytes
(tests/golden/jitter.npz, written by tests/golden/make_jitter_golden.py) bit for bit and against the PIL installed here, the host half of
the Python layer (draw_jitter, the step tables), the deliberate mistakes the fixture must catch, and the refusals of the two entries."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import crop_ref as C
import fold_ref as R
import jitter_ref as J
import sstem_native


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "jitter.npz")))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _blend_rows(variant=None):
    """The restatement of fixture (a): [factor, d, 256]."""
    ramp = np.arange(256)
    return np.stack([np.stack([J.blend(d, ramp, f, variant) for d in range(256)]) for f in J.BLEND_FACTORS]).astype(np.uint8)


def _provider_sample(seed, variant=None):
    """Fixture (c) restated: crop_ref's draws and crops, the jitter's draws, the table, then the rejection loop on fold_ref."""
    images = C.images_of(C.FUSION_IMAGES)
    shapes = [images[p[0]].shape for p in C.FUSION_PAIRS]
    rng = random.Random(seed)
    clean, interp = C.fusion_crops(images, C.FUSION_PAIRS, C.draw_sample(rng, C.FUSION_FLAGS, shapes, C.FUSION_CROP), C.FUSION_CROP)
    steps = J.draw_jitter(rng, *J.PROVIDER_JITTER)
    lut = J.lut_of(clean, steps, variant)
    off = (C.FUSION_CROP[0] - C.FUSION_DET) // 2
    drawn = 0
    while True:
        fold = R.draw_fold(rng, C.FUSION_CROP[0], C.FUSION_CROP[0])
        drawn += 1
        got = J.degrade(clean, interp, R.scalars(*fold), (off, off, C.FUSION_DET, C.FUSION_DET), lut, bool(seed & 1))
        if got["zero_count"] >= 100:
            return got, steps, drawn, rng.random()


# ---- the restatement against PIL's recorded bytes --------------------------------------------------------------------------------------
def test_blend_equals_pil_on_every_byte(golden):
    got, want = _blend_rows(), golden["blend"]
    assert want.shape == (len(J.BLEND_FACTORS), 256, 256)
    assert _same(got, want), "%d of %d bytes differ" % (int((got != want).sum()), want.size)


@pytest.mark.parametrize("chain", range(len(J.CHAINS)))
def test_chains_equal_pil_at_every_pixel(golden, chain):
    for name, img in J.images().items():
        want = golden["c%d_%s" % (chain, name)]
        got = J.apply(img, J.CHAINS[chain])
        assert _same(got, want), "chain %d on %s: %d pixels differ" % (chain, name, int((got != want).sum()))


def test_fixture_covers_the_edge_cases(golden):
    imgs = J.images()
    assert imgs["one"].shape == (1, 1) and imgs["zeros"].max() == 0 and imgs["full"].min() == 255
    assert 2 * int(imgs["half"].sum()) == 201 * imgs["half"].size                                  # the mean is 100.5 exactly
    below = imgs["below_half"]
    assert 0 < below.size * 201 - 2 * int(below.sum()) <= 2                                        # ... and here just below it
    assert J.mean_byte(np.bincount(imgs["half"].ravel(), minlength=256), imgs["half"].size, np.arange(256)) == 101
    assert J.mean_byte(np.bincount(below.ravel(), minlength=256), below.size, np.arange(256)) == 100
    assert np.count_nonzero(np.bincount(imgs["em"].ravel(), minlength=256)) < 110                  # a narrow histogram
    assert {0.6, 1.1, 1.3} <= set(J.BLEND_FACTORS) and np.float32(J.BLEND_FACTORS[-1]) > 1
    orders = {tuple(c for c, _ in chain) for chain in J.CHAINS[:6]}
    assert len(orders) == 6 and all(sorted(o) == [1, 2, 3] for o in orders)
    assert all(len(chain) <= J.OPS for chain in J.CHAINS) and len(J.CHAINS[7]) == 4
    assert max(int(golden["p%d_drawn" % s]) for s in J.PROVIDER_SEEDS) > 1 and min(int(golden["p%d_drawn" % s]) for s in J.PROVIDER_SEEDS) == 1
    # saturation is the identity on a mode-L image: a chain without it gives the recorded bytes too
    for ci, chain in enumerate(J.CHAINS[:6]):
        assert _same(J.apply(imgs["noise"], [s for s in chain if s[0] != J.SATURATION]), golden["c%d_noise" % ci])


@pytest.mark.parametrize("seed", J.PROVIDER_SEEDS)
def test_provider_sample_reproduces_the_reference(golden, seed):
    got, steps, drawn, after = _provider_sample(seed)
    key = "p%d_" % seed
    assert np.array_equal(np.array(steps, dtype=np.float64), golden[key + "steps"])
    assert drawn == int(golden[key + "drawn"]) and after == float(golden[key + "next"])
    assert _same(got["im"], golden[key + "im"]) and _same(got["lb"], golden[key + "lb"])


def test_live_pil_agrees_with_the_fixture_and_the_restatement(golden):
    PIL = pytest.importorskip("PIL")
    from PIL import Image, ImageEnhance
    enhancers = {J.BRIGHTNESS: ImageEnhance.Brightness, J.CONTRAST: ImageEnhance.Contrast, J.SATURATION: ImageEnhance.Color}
    ramp = Image.fromarray(np.arange(256, dtype=np.uint8)[None, :])
    for fi, f in enumerate(J.BLEND_FACTORS):
        for d in (0, 1, 77, 128, 254, 255):
            live = np.asarray(Image.blend(Image.new("L", (256, 1), d), ramp, f))[0]
            assert np.array_equal(live, golden["blend"][fi, d]), (PIL.__version__, str(golden["pil_version"]), f, d)
    rng = random.Random(5)
    img = J.images()["noise"]
    for _ in range(20):                                    # chains the fixture does not hold: random factors, random order
        steps = J.draw_jitter(rng, 0.5, 0.5, 0.5)
        pil = Image.fromarray(img)
        for code, factor in steps:
            pil = enhancers[code](pil).enhance(factor)
        assert np.array_equal(np.asarray(pil), J.apply(img, steps)), steps


# ---- the mutants -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", J.MUTANTS)
def test_fixture_catches_the_mutant(golden, variant):
    """Each deliberate mistake changes at least one recorded byte (and the unmutated restatement changes none, above)."""
    caught = []
    if not _same(_blend_rows(variant), golden["blend"]):
        caught.append("blend")
    for ci, chain in enumerate(J.CHAINS):
        for name, img in J.images().items():
            if not _same(J.apply(img, chain, variant), golden["c%d_%s" % (ci, name)]):
                caught.append("c%d_%s" % (ci, name))
    for seed in J.PROVIDER_SEEDS:
        got = _provider_sample(seed, variant)[0]
        if not _same(got["im"], golden["p%d_im" % seed]):
            caught.append("p%d" % seed)
    assert caught, "nothing in the fixture tells %s from the contract" % variant
    assert len(J.MUTANTS) >= 5


def test_arithmetic_mutants_are_caught_by_the_blend_table_alone(golden):
    """The factors the blend table was given tell fused and double arithmetic from float32 without any image."""
    for variant in ("fused_multiply", "double_factor", "rounded_bytes"):
        assert not _same(_blend_rows(variant), golden["blend"]), variant


# ---- the host half of the Python layer -------------------------------------------------------------------------------------------------
def test_draw_jitter_consumes_the_stream_like_the_literal_draws():
    from data.color_jitter import draw_jitter
    a, b = random.Random(31), random.Random(31)
    for _ in range(50):
        got = draw_jitter(a, 0.5, 0.5, 0.5)
        want = [(1, b.uniform(0.5, 1.5)), (2, b.uniform(0.5, 1.5)), (3, b.uniform(0.5, 1.5))]
        b.shuffle(want)
        assert got == want
    assert a.random() == b.random()
    # a zero strength draws nothing; a strength above 1 starts at 0
    got = draw_jitter(a, 0.0, 1.5, 0.0)
    want = [(2, b.uniform(0, 2.5))]
    b.shuffle(want)
    assert got == want and a.random() == b.random()
    assert draw_jitter(a, 0, 0, 0) == [] and a.random() == b.random()      # shuffling an empty list draws nothing
    # the restatement's draws are the package's
    for _ in range(20):
        assert draw_jitter(a, 0.5, 0.25, 0.5) == J.draw_jitter(b, 0.5, 0.25, 0.5)


def test_step_tables_validate_on_the_host():
    from data import color_jitter
    assert color_jitter.JITTER_OPS == J.OPS == 4
    assert (color_jitter.NONE, color_jitter.BRIGHTNESS, color_jitter.CONTRAST, color_jitter.SATURATION) == (0, 1, 2, 3)
    steps = [[(1, 0.6), (2, 1.1)], [], [(3, 0.5), (2, 1.3), (1, 0.7), (2, 0.9)]]
    codes, factors = color_jitter.step_tables(steps)
    want = J.step_arrays(steps)
    assert codes.dtype == np.int32 and factors.dtype == np.float32 and np.array_equal(codes, want[0]) and np.array_equal(factors, want[1])
    with pytest.raises(ValueError):
        color_jitter.step_tables([[(4, 1.0)]])
    with pytest.raises(ValueError):
        color_jitter.step_tables([[(-1, 1.0)]])
    with pytest.raises(ValueError):
        color_jitter.step_tables([[(1, 1.0)] * 5])
    with pytest.raises(NotImplementedError):
        color_jitter.jitter_luts(torch.zeros((1, 4, 4), dtype=torch.uint8), [[]])
    from data.fold_degradation import FoldBatch
    batch = FoldBatch(0, (0, 0, 4, 4), "image", "cpu")
    assert batch.lut is None and batch.jitter_steps is None


# ---- the library ---------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_two_entries():
    lib = ctypes.CDLL(sstem_native.library_path())
    for name in ("sstem_jitter_lut_u8", "sstem_fold_degrade_lut_u8"):
        assert hasattr(lib, name) and name in sstem_native.C_ABI


_P = 64          # a non-null "pointer" that is never dereferenced: every call below is refused, or is a no-op, before any HIP call


def test_argument_validation_without_gpu():
    lib = sstem_native.load_library()

    def refused(rc, status, text):
        assert rc == status and lib.sstem_last_error().decode() == text, (rc, lib.sstem_last_error())

    lut, deg = lib.sstem_jitter_lut_u8, lib.sstem_fold_degrade_lut_u8
    # (planes, n, S_h, S_w, op_code, op_factor, lut, hist, stream)
    assert lut(None, 0, 40, 56, None, None, None, None, None) == 0                 # n == 0 and an empty plane: successful no-ops
    assert lut(None, 3, 0, 56, None, None, None, None, None) == 0 and lut(None, 3, 40, 0, None, None, None, None, None) == 0
    for i in range(5):
        ptrs = [_P] * 5
        ptrs[i] = None
        refused(lut(ptrs[0], 1, 40, 56, *ptrs[1:], None), 1, "jitter lut: null plane, step table, lut or hist")
    for bad in ((-1, 40, 56), (1, -40, 56), (1, 40, -56)):
        refused(lut(_P, *bad, _P, _P, _P, _P, None), 2, "jitter lut: negative size")
    for big in ((1, 32769, 56), (1, 40, 32769), ((1 << 24) + 1, 40, 56)):
        refused(lut(_P, *big, _P, _P, _P, _P, None), 3, "jitter lut: sizes past the index range (S_h, S_w <= 32768, n <= 2^24)")
    # (clean, interp, folds, slot, n, slots, S_h, S_w, off_y, off_x, out_h, out_w, gt_line, lut, deformed, flow2, im, lb, zero_count, stream):
    # what sstem_fold_degrade_u8 refuses, with and without a table
    outs = (_P, _P, _P, _P, _P)
    for table in (None, _P):
        assert deg(None, None, None, None, 0, 4, 64, 64, 8, 8, 48, 48, 0, table, None, None, None, None, None, None) == 0
        assert deg(_P, _P, _P, None, 2, 4, 64, 64, 8, 8, 48, 48, 1, table, None, None, None, None, None, None) == 0     # no output asked for
        refused(deg(None, _P, _P, None, 1, 1, 64, 64, 8, 8, 48, 48, 0, table, *outs, None), 1, "fold degrade (lut): null plane or fold table")
        refused(deg(_P, _P, None, None, 1, 1, 64, 64, 8, 8, 48, 48, 0, table, *outs, None), 1, "fold degrade (lut): null plane or fold table")
        refused(deg(_P, None, _P, None, 1, 1, 64, 64, 8, 8, 48, 48, 0, table, *outs, None), 1, "fold degrade (lut): im needs the interp plane")
        for i in range(8):
            sizes = [1, 1, 64, 64, 8, 8, 48, 48]
            sizes[i] = -sizes[i]
            refused(deg(_P, _P, _P, None, *sizes, 0, table, *outs, None), 2, "fold degrade (lut): negative size")
        for window in ((8, 8, 57, 48), (8, 8, 48, 57), (65, 0, 0, 0), (0, 17, 48, 48), (0, 0, 65, 64)):
            refused(deg(_P, _P, _P, None, 1, 1, 64, 64, *window, 0, table, *outs, None), 2, "fold degrade (lut): the window is not inside the plane")
        for n, slots, sh, sw in (((1 << 24) + 1, 1, 64, 64), (1, (1 << 24) + 1, 64, 64), (1, 1, 32769, 64), (1, 1, 64, 32769)):
            refused(deg(_P, _P, _P, None, n, slots, sh, sw, 8, 8, 48, 48, 0, table, *outs, None), 3,
                    "fold degrade (lut): sizes past the index range (S_h, S_w <= 32768, n, slots <= 2^24)")
