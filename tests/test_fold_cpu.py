"""Fold synthesis without a GPU: the numpy restatement of the contract (tests/fold_ref.py) against the reference's fixture
(tests/golden/fold.npz, written by tests/golden/make_fold_golden.py) bit for bit, the host half of the Python layer (draw_fold,
fold_scalars, the rejection rule), the deliberate mistakes the fixture must catch, and the refusals of the three entry points."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import fold_ref as R
import sstem_native
from data.fold_degradation import draw_fold
from utils import flow_synthesis
from utils.image_warp import image_warp


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "fold.npz")))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _case(golden, name, variant=None):
    """fold_ref on the recorded doubles of fold `name` -> dict of the fixture's five arrays."""
    H, W, _, img = R.fold_case(name)
    row = golden[name + "_row"]
    flow, flow2, mask = R.flow(row, H, W, variant=variant)
    bil = R.warp(img, flow, "bilinear", variant=variant)
    return {"flow": flow, "flow2": flow2, "mask": mask, "warp_bilinear": bil, "warp_nearest": R.warp(img, flow, "nearest", variant=variant),
            "deformed": bil * mask}


@pytest.mark.parametrize("name", list(R.FOLD_CASES))
def test_restatement_equals_the_reference_bit_for_bit(golden, name):
    got = _case(golden, name)
    for key, value in got.items():
        want = golden[name + "_" + key]
        assert _same(value, want), "%s %s: %d elements differ" % (name, key, int((_bits(value) != _bits(want)).sum()))


def test_fixture_covers_the_edge_cases(golden):
    """What the cases were chosen for is really in the file: exact ties of both comparisons, d == 0, negative zeros, clamped taps."""
    row = golden["k0_ties_row"]
    assert row[0] == 0.0 and row[1] == 17.0 and row[2] == 1.0
    m = golden["k0_ties_mask"]
    assert m[12].max() == 0 and m[11].min() == 1 and m[22].max() == 0 and m[23].min() == 1      # a == line_width is inside the line
    f2 = golden["k0_ties_flow2"]
    assert np.signbit(f2[17]).any() and (f2[17] == 0).all()                                       # d == 0: dis2 = s2 * (-0.0)
    assert any((np.signbit(golden[n + "_flow"]) & (golden[n + "_flow"] == 0)).any() for n in R.FOLD_CASES)
    assert golden["zero_den_row"][0] == 40 / 1e-9 and golden["wide_20_80_row"][3] == 20 and golden["wide_20_80_row"][4] == 80
    assert golden["fw_lw_plus1_row"][4] == golden["fw_lw_plus1_row"][3] + 1
    assert golden["non_square_flow"].shape == (33, 61, 2)
    fl = golden["wide_20_80_flow"]
    xs = np.arange(56)[None, :] + np.floor(fl[..., 0])
    assert (xs < 0).any() or (xs > 55).any()                                                      # taps clamped at the border


def test_scalars_of_the_package_are_the_restatement_s():
    for name in R.FOLD_CASES:
        fold = R.fold_case(name)[2]
        assert np.array_equal(np.array(flow_synthesis.fold_scalars(*fold), dtype=np.float64), R.scalars(*fold)), name
    assert flow_synthesis.gen_line([0, 10], [40, 10]) == R.gen_line([0, 10], [40, 10]) == (40 / 1e-9, 0 - (40 / 1e-9) * 10)
    assert flow_synthesis.FOLD_PARAMS == R.PARAMS == 10


def test_draw_fold_consumes_the_stream_like_the_restatement():
    a, b = random.Random(77), random.Random(77)
    for _ in range(200):
        assert draw_fold(a, 64, 48) == R.draw_fold(b, 64, 48)
    assert a.random() == b.random()


@pytest.mark.parametrize("seed", R.DEGRADE_SEEDS)
def test_rejection_loop_reproduces_the_reference(golden, seed):
    """draw_fold + fold_ref + the rejection rule against what Train.degradation returned after random.seed(seed)."""
    clean = R.image(R.DEGRADE_IMAGE_SEED, R.DEGRADE_SIZE, R.DEGRADE_SIZE)
    rng = random.Random(seed)
    off = R.DEGRADE_OFFSET
    window = (off, off, R.DEGRADE_SIZE - 2 * off, R.DEGRADE_SIZE - 2 * off)
    drawn = 0
    while True:
        fold = draw_fold(rng, R.DEGRADE_SIZE, R.DEGRADE_SIZE)
        drawn += 1
        got = R.degrade(clean, None, R.scalars(*fold), window)
        if got["zero_count"] >= R.DEGRADE_MIN_ZERO:
            break
    key = "s%d_" % seed
    assert drawn == int(golden[key + "drawn"])
    assert _same(got["deformed"], golden[key + "deformed"])
    assert _same(got["flow2"], np.ascontiguousarray(np.transpose(golden[key + "flow2"], (2, 0, 1))))


def test_fixture_has_a_rejecting_and_an_accepting_seed(golden):
    drawn = [int(golden["s%d_drawn" % s]) for s in R.DEGRADE_SEEDS]
    assert min(drawn) == 1 and max(drawn) > 1


@pytest.mark.parametrize("variant", R.MUTANTS)
def test_fixture_catches_the_mutant(golden, variant):
    """Each deliberate mistake changes at least one bit of at least one case (and the unmutated restatement changes none, above)."""
    caught = []
    for name in R.FOLD_CASES:
        got = _case(golden, name, variant)
        if not all(_same(value, golden[name + "_" + key]) for key, value in got.items()):
            caught.append(name)
    assert caught, "no fold of the fixture tells %s from the contract" % variant
    assert len(R.MUTANTS) >= 5


def test_library_exports_the_three_entries():
    lib = ctypes.CDLL(sstem_native.library_path())
    for name in ("sstem_fold_flow", "sstem_image_warp_u8", "sstem_fold_degrade_u8"):
        assert hasattr(lib, name) and name in sstem_native.C_ABI


_P = 64          # a non-null "pointer" that is never dereferenced: every call below is refused, or is a no-op, before any HIP call


def test_argument_validation_without_gpu():
    lib = sstem_native.load_library()

    def refused(rc, status, text):
        assert rc == status and lib.sstem_last_error().decode() == text, (rc, lib.sstem_last_error())

    flow, warp, deg = lib.sstem_fold_flow, lib.sstem_image_warp_u8, lib.sstem_fold_degrade_u8
    # (folds, n, H, W, flow, flow2, mask, stream)
    assert flow(None, 0, 40, 56, None, None, None, None) == 0                    # n == 0: a successful no-op
    assert flow(None, 1, 0, 56, None, None, None, None) == 0 and flow(_P, 1, 40, 56, None, None, None, None) == 0
    refused(flow(None, 1, 40, 56, _P, _P, _P, None), 1, "fold flow: null fold table")
    for bad in ((-1, 40, 56), (1, -40, 56), (1, 40, -56)):
        refused(flow(_P, *bad, _P, _P, _P, None), 2, "fold flow: negative size")
    for big in ((1, 32769, 56), (1, 40, 32769), ((1 << 24) + 1, 40, 56)):
        refused(flow(_P, *big, _P, _P, _P, None), 3, "fold flow: sizes past the index range (H, W <= 32768, n <= 2^24)")
    # (im, flow, out, n, H, W, C, mode, stream)
    assert warp(None, None, None, 0, 40, 56, 1, 1, None) == 0 and warp(None, None, None, 2, 40, 0, 3, 0, None) == 0
    for nulls in ((None, _P, _P), (_P, None, _P), (_P, _P, None)):
        refused(warp(*nulls, 1, 40, 56, 1, 1, None), 1, "image warp (u8): null tensor pointer")
    for bad in ((-1, 40, 56), (1, -40, 56), (1, 40, -56)):
        refused(warp(_P, _P, _P, *bad, 1, 1, None), 2, "image warp (u8): negative size")
    for c in (0, -3):
        refused(warp(_P, _P, _P, 1, 40, 56, c, 1, None), 2, "image warp (u8): C must be at least 1")
    for mode in (-1, 2, 7):
        refused(warp(_P, _P, _P, 1, 40, 56, 1, mode, None), 3, "image warp (u8): unknown mode")
    for big in ((1, 32769, 56, 1), (1, 40, 56, 1025), ((1 << 24) + 1, 40, 56, 1)):
        refused(warp(_P, _P, _P, *big, 1, None), 3, "image warp (u8): sizes past the index range (H, W <= 32768, n <= 2^24, C <= 1024)")
    # (clean, interp, folds, slot, n, slots, S_h, S_w, off_y, off_x, out_h, out_w, gt_line, deformed, flow2, im, lb, zero_count, stream)
    outs = (_P, _P, _P, _P, _P)
    assert deg(None, None, None, None, 0, 4, 64, 64, 8, 8, 48, 48, 0, None, None, None, None, None, None) == 0
    assert deg(_P, _P, _P, None, 2, 4, 64, 64, 8, 8, 48, 48, 1, None, None, None, None, None, None) == 0        # no output asked for
    refused(deg(None, _P, _P, None, 1, 1, 64, 64, 8, 8, 48, 48, 0, *outs, None), 1, "fold degrade: null plane or fold table")
    refused(deg(_P, _P, None, None, 1, 1, 64, 64, 8, 8, 48, 48, 0, *outs, None), 1, "fold degrade: null plane or fold table")
    refused(deg(_P, None, _P, None, 1, 1, 64, 64, 8, 8, 48, 48, 0, *outs, None), 1, "fold degrade: im needs the interp plane")
    for i in range(8):
        sizes = [1, 1, 64, 64, 8, 8, 48, 48]
        sizes[i] = -sizes[i]
        refused(deg(_P, _P, _P, None, *sizes, 0, *outs, None), 2, "fold degrade: negative size")
    for window in ((8, 8, 57, 48), (8, 8, 48, 57), (65, 0, 0, 0), (0, 65, 0, 0), (17, 0, 48, 48), (0, 17, 48, 48), (0, 0, 65, 64)):
        refused(deg(_P, _P, _P, None, 1, 1, 64, 64, *window, 0, *outs, None), 2, "fold degrade: the window is not inside the plane")
    for n, slots, sh, sw in (((1 << 24) + 1, 1, 64, 64), (1, (1 << 24) + 1, 64, 64), (1, 1, 32769, 64), (1, 1, 64, 32769)):
        refused(deg(_P, _P, _P, None, n, slots, sh, sw, 8, 8, 48, 48, 0, *outs, None), 3,
                "fold degrade: sizes past the index range (S_h, S_w <= 32768, n, slots <= 2^24)")


def test_python_layer_refuses_host_arrays():
    with pytest.raises(NotImplementedError):
        image_warp(np.zeros((4, 4), np.uint8), np.zeros((4, 4, 2), np.float32))
    with pytest.raises(NotImplementedError):
        image_warp(torch.zeros((4, 4), dtype=torch.uint8), torch.zeros((4, 4, 2)))
    with pytest.raises(NotImplementedError):
        flow_synthesis.gen_flow(8, 8, 1.0, 0.0, device="cpu")
    from data.fold_degradation import degrade
    with pytest.raises(NotImplementedError):
        degrade(torch.zeros((1, 8, 8), dtype=torch.uint8), None, [(1.0, 0.0, 5, 10, 0.1)], (0, 0, 8, 8))
