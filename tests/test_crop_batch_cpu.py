"""Training crops without a GPU: the numpy restatement of the contract (tests/crop_ref.py) against the reference providers' fixture
(tests/golden/crop_batch.npz, written by tests/golden/make_crop_batch_golden.py) bit for bit, the host half of the Python layer
(orientation_code, SP_ROTATION_FLIP, the draws), the deliberate mistakes the fixture must catch, and the refusals of the two entries."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import crop_ref as C
import sstem_native
from data.fold_degradation import draw_fold, draw_fusion_crop
from data.interp_batch import draw_interp_sample
from data.resident import SP_ROTATION_FLIP, AugFlags, ResidentImages, crop_u8, orientation_code


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "crop_batch.npz")))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _interp_cases():
    for fname, flags in C.INTERP_FLAG_SETS.items():
        for seed in C.INTERP_SEEDS if fname == "all" else C.INTERP_SEEDS[:C.INTERP_OTHER_SEEDS]:
            yield fname, flags, seed


INTERP_SHAPES = [(C.INTERP_IMAGES[t[0]][1], C.INTERP_IMAGES[t[0]][2]) for t in C.INTERP_TRIPLETS]
FUSION_SHAPES = [(C.FUSION_IMAGES[p[0]][1], C.FUSION_IMAGES[p[0]][2]) for p in C.FUSION_PAIRS]


def test_orientation_code_against_numpy():
    """All 2 * 2 * 2 * 4 draw combinations on a non-symmetric square: the provider's sequence equals the kernel's form of the code."""
    sq = C.image(1, 5, 5)
    seen = set()
    for lr in (False, True):
        for ud in (False, True):
            for z in (False, True):
                for r in range(4):
                    m = sq
                    if lr:
                        m = np.fliplr(m)
                    if ud:
                        m = np.flipud(m)
                    if z:
                        m = np.transpose(m)
                    m = np.rot90(m, r)
                    code = orientation_code(lr, ud, z, r)
                    assert 0 <= code < 8 and np.array_equal(C.orient(sq, code), m), (lr, ud, z, r, code)
                    assert code == C.orientation_code(lr, ud, z, r)
                    seen.add(code)
    assert seen == set(range(8))
    assert len({C.orient(sq, code).tobytes() for code in range(8)}) == 8


def test_sp_rotation_flip_against_the_fixture(golden):
    square = C.image(*C.SP_SQUARE)
    assert len(SP_ROTATION_FLIP) == 8
    for case in range(8):
        assert np.array_equal(C.orient(square, SP_ROTATION_FLIP[case]), golden["sp_case"][case]), case


@pytest.mark.parametrize("fname,flags,seed", list(_interp_cases()))
def test_interp_restatement_and_draws(golden, fname, flags, seed):
    """crop_ref equals the reference's im and lb bit for bit, and both statements of the draws leave the stream where __getitem__ left it."""
    key = "i_%s_%d_" % (fname, seed)
    images = C.images_of(C.INTERP_IMAGES)
    rng = random.Random(seed)
    draw = C.draw_sample(rng, flags, INTERP_SHAPES, C.INTERP_CROP)
    assert rng.random() == float(golden[key + "next"])
    im, lb = C.interp_sample(images, C.INTERP_TRIPLETS, draw, C.INTERP_CROP)
    assert _same(im, golden[key + "im"]) and _same(lb, golden[key + "lb"])
    rng = random.Random(seed)
    k, i, j, code, swap = draw_interp_sample(rng, AugFlags(*flags), INTERP_SHAPES, C.INTERP_CROP)
    assert rng.random() == float(golden[key + "next"])
    assert (k, i, j, code, swap) == (draw[0], draw[1], draw[2], C.orientation_code(*draw[3]), draw[4])


def _fusion_reference(images, seed, rng):
    """draw_sample + crop_ref + the existing fold restatement's rejection loop -> im, lb of the fusion provider."""
    import fold_ref as R
    draw = C.draw_sample(rng, C.FUSION_FLAGS, FUSION_SHAPES, C.FUSION_CROP)
    clean, interp = C.fusion_crops(images, C.FUSION_PAIRS, draw, C.FUSION_CROP)
    S = C.FUSION_CROP[0]
    off = (S - C.FUSION_DET) // 2
    while True:
        got = R.degrade(clean, interp, R.scalars(*R.draw_fold(rng, S, S)), (off, off, C.FUSION_DET, C.FUSION_DET), gt_line=bool(seed & 1))
        if got["zero_count"] >= 100:
            return got["im"], got["lb"]


@pytest.mark.parametrize("seed", C.FUSION_SEEDS)
def test_fusion_restatement_and_draws(golden, seed):
    key = "f_%d_" % seed
    images = C.images_of(C.FUSION_IMAGES)
    rng = random.Random(seed)
    im, lb = _fusion_reference(images, seed, rng)
    assert rng.random() == float(golden[key + "next"])
    assert _same(im, golden[key + "im"]) and _same(lb, golden[key + "lb"])
    # the package's draws: the crop, then folds until the restatement's count accepts one
    import fold_ref as R
    rng, ref = random.Random(seed), random.Random(seed)
    k, i, j, code = draw_fusion_crop(rng, AugFlags(*C.FUSION_FLAGS), FUSION_SHAPES, C.FUSION_CROP)
    d = C.draw_sample(ref, C.FUSION_FLAGS, FUSION_SHAPES, C.FUSION_CROP)
    assert (k, i, j, code) == (d[0], d[1], d[2], C.orientation_code(*d[3])) and rng.getstate() == ref.getstate()
    assert draw_fold(rng, 100, 100) == R.draw_fold(ref, 100, 100)


def test_fusion_swap_is_refused():
    with pytest.raises(ValueError):
        draw_fusion_crop(random.Random(0), AugFlags(True, True, True, True, True), FUSION_SHAPES, C.FUSION_CROP)


def test_disabled_augmentations_draw_nothing():
    rng, ref = random.Random(5), random.Random(5)
    k, i, j, code, swap = draw_interp_sample(rng, AugFlags(False, False, False, False, False), INTERP_SHAPES, C.INTERP_CROP)
    H, W = INTERP_SHAPES[ref.randint(0, len(INTERP_SHAPES) - 1)]
    ref.randint(0, H - C.INTERP_CROP[0]), ref.randint(0, W - C.INTERP_CROP[1])
    assert rng.getstate() == ref.getstate() and code == 0 and swap is False


@pytest.mark.parametrize("variant", C.MUTANTS)
def test_fixture_catches_the_mutant(golden, variant):
    """Each deliberate mistake changes at least one bit of at least one interp sample (the unmutated restatement changes none, above)."""
    images = C.images_of(C.INTERP_IMAGES)
    caught = 0
    for fname, flags, seed in _interp_cases():
        key = "i_%s_%d_" % (fname, seed)
        draw = C.draw_sample(random.Random(seed), flags, INTERP_SHAPES, C.INTERP_CROP)
        try:
            im, lb = C.interp_sample(images, C.INTERP_TRIPLETS, draw, C.INTERP_CROP, variant)
        except (ValueError, IndexError):                   # an exchanged origin may fall outside the image
            caught += 1
            continue
        if not (_same(im, golden[key + "im"]) and _same(lb, golden[key + "lb"])):
            caught += 1
    assert caught, "no sample of the fixture tells %s from the contract" % variant
    assert len(C.MUTANTS) == 5


def test_fixture_covers_codes_swaps_and_sizes():
    codes, swaps, ks = set(), set(), set()
    for seed in C.INTERP_SEEDS:
        d = C.draw_sample(random.Random(seed), C.ALL_FLAGS, INTERP_SHAPES, C.INTERP_CROP)
        codes.add(C.orientation_code(*d[3])), swaps.add(d[4]), ks.add(d[0])
    assert codes == set(range(8)) and swaps == {False, True} and ks == {0, 1, 2}


def test_restatement_skips_the_samples_that_write_nothing():
    images = [C.image(1, 20, 24), C.image(2, 24, 20)]
    samples = [(0, 0, 0), (1, 0, 0), (0, 0, 8), (0, 0, -1), (0, 0, 0), (0, 0, 0), (-1, 0, 0), (0, 0, 3)]
    planes = [(0, 1), (0, 1), (0, 1), (0, 1), (0, 2), (-1, 0), (0, 0), (1, 0)]
    out = C.crop_u8(images, samples, planes, 20, 20, out=np.full((2, 8, 20, 20), 0xAB, np.uint8))
    written = [bool((out[:, i] != 0xAB).any()) for i in range(8)]
    assert written == [True, False, False, False, False, False, False, True]
    assert not C.sample_writes(images, (0,), 0, 0, 4, 20, 24) and C.sample_writes(images, (0,), 0, 0, 3, 20, 24)


def test_library_exports_the_two_entries():
    lib = ctypes.CDLL(sstem_native.library_path())
    for name in ("sstem_crop_orient_u8", "sstem_crop_orient_f32"):
        assert hasattr(lib, name) and name in sstem_native.C_ABI


_P = 64          # a non-null "pointer" that is never dereferenced: every call below is refused, or is a no-op, before any HIP call


def test_argument_validation_without_gpu():
    lib = sstem_native.load_library()

    def refused(rc, status, text):
        assert rc == status and lib.sstem_last_error().decode() == text, (rc, lib.sstem_last_error())

    u8, f32 = lib.sstem_crop_orient_u8, lib.sstem_crop_orient_f32
    chan = (ctypes.c_int32 * 7)(0, 0, 0, 2, 2, 2, 1)
    tabs = (_P, _P, 4, _P, _P)                             # pool, images, n_images, samples, plane_image
    # (pool, images, n_images, samples, plane_image, n, P, S_h, S_w, out, stream)
    assert u8(None, None, 0, None, None, 0, 3, 40, 40, None, None) == 0                      # n == 0: a successful no-op
    assert u8(None, None, 4, None, None, 2, 3, 0, 40, None, None) == 0 and u8(None, None, 4, None, None, 2, 3, 40, 0, None, None) == 0
    for i in range(4):
        nulls = list(tabs)
        nulls[i if i < 2 else i + 1] = None
        refused(u8(*nulls, 2, 3, 40, 40, _P, None), 1, "crop orient (u8): null pool or table")
    refused(u8(*tabs, 2, 3, 40, 40, None, None), 1, "crop orient (u8): null output")
    for bad in ((-1, 3, 40, 40), (2, 3, -40, 40), (2, 3, 40, -40)):
        refused(u8(*tabs, *bad, _P, None), 2, "crop orient (u8): negative size")
    refused(u8(_P, _P, -1, _P, _P, 2, 3, 40, 40, _P, None), 2, "crop orient (u8): negative size")
    for p in (0, -2):
        refused(u8(*tabs, 2, p, 40, 40, _P, None), 2, "crop orient (u8): P must be at least 1")
    refused(u8(*tabs, 2, 17, 40, 40, _P, None), 3, "crop orient (u8): more than 16 planes or channels")
    assert u8(None, None, 4, None, None, 0, 16, 40, 40, None, None) == 0
    for big in (((1 << 24) + 1, 3, 40, 40), (2, 3, 32769, 40), (2, 3, 40, 32769)):
        refused(u8(*tabs, *big, _P, None), 3, "crop orient (u8): sizes past the index range (S_h, S_w <= 32768, n, n_images <= 2^24)")
    refused(u8(_P, _P, (1 << 24) + 1, _P, _P, 2, 3, 40, 40, _P, None), 3,
            "crop orient (u8): sizes past the index range (S_h, S_w <= 32768, n, n_images <= 2^24)")
    # (pool, images, n_images, samples, plane_image, n, P, S_h, S_w, chan_plane, C0, C1, chan_invert, out0, out1, stream)
    assert f32(None, None, 0, None, None, 0, 3, 40, 40, None, 6, 1, 0, None, None, None) == 0
    assert f32(None, None, 4, None, None, 2, 3, 40, 0, None, 6, 1, 0, None, None, None) == 0
    for i in range(4):
        nulls = list(tabs)
        nulls[i if i < 2 else i + 1] = None
        refused(f32(*nulls, 2, 3, 40, 40, chan, 6, 1, 0, _P, _P, None), 1, "crop orient (f32): null pool or table")
    for ptrs in ((None, _P, _P), (chan, None, _P), (chan, _P, None)):
        refused(f32(*tabs, 2, 3, 40, 40, ptrs[0], 6, 1, 0, ptrs[1], ptrs[2], None), 1, "crop orient (f32): null channel map or output")
    for bad in ((-1, 3, 40, 40, 6, 1), (2, 3, -40, 40, 6, 1), (2, 3, 40, -40, 6, 1), (2, 3, 40, 40, -6, 1), (2, 3, 40, 40, 6, -1)):
        refused(f32(*tabs, *bad[:4], chan, bad[4], bad[5], 0, _P, _P, None), 2, "crop orient (f32): negative size")
    refused(f32(*tabs, 2, 0, 40, 40, chan, 6, 1, 0, _P, _P, None), 2, "crop orient (f32): P must be at least 1")
    refused(f32(*tabs, 2, 3, 40, 40, chan, 0, 1, 0, _P, _P, None), 2, "crop orient (f32): C0 must be at least 1")
    refused(f32(*tabs, 2, 17, 40, 40, chan, 6, 1, 0, _P, _P, None), 3, "crop orient (f32): more than 16 planes or channels")
    refused(f32(*tabs, 2, 3, 40, 40, chan, 16, 1, 0, _P, _P, None), 3, "crop orient (f32): more than 16 planes or channels")
    refused(f32(*tabs, (1 << 24) + 1, 3, 40, 40, chan, 6, 1, 0, _P, _P, None), 3,
            "crop orient (f32): sizes past the index range (S_h, S_w <= 32768, n, n_images <= 2^24)")
    for entries in ((0, 0, 0, 2, 2, 3, 1), (0, 0, 0, 2, 2, 2, -1)):
        refused(f32(*tabs, 2, 3, 40, 40, (ctypes.c_int32 * 7)(*entries), 6, 1, 0, _P, _P, None), 2,
                "crop orient (f32): a channel's plane is outside [0, P)")
    refused(f32(*tabs, 2, 2, 40, 40, chan, 6, 0, 0, _P, None, None), 2, "crop orient (f32): a channel's plane is outside [0, P)")


def test_python_layer_refuses_the_cpu():
    with pytest.raises(NotImplementedError):
        ResidentImages([np.zeros((4, 4), np.uint8)], "cpu")
    with pytest.raises(NotImplementedError):
        crop_u8(torch.zeros((4, 4), dtype=torch.uint8), None, 2, 2)
    from data.sp_patches import sp_patches
    with pytest.raises(NotImplementedError):
        sp_patches(None, [], [], [], 8, if_bdadjust=True)
