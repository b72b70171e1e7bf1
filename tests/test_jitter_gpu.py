"""Colour jitter on the GPU (include/sstem_jitter.h and its Python layer), every comparison bit for bit: the table entry against PIL's
recorded bytes (tests/golden/jitter.npz) and, at every one of the 256 entries, against the numpy restatement tests/jitter_ref.py; the
degrade entry that reads through a table against sstem_fold_degrade_u8 run on the host-jittered plane; the batchers against the
fusion provider's recorded sample.  The file reads the fixture and never PIL."""
import os
import random

import numpy as np
import pytest
import torch

import crop_ref as C
import fold_ref as R
import jitter_ref as J
import sstem_native
from data.color_jitter import jitter_luts
from data.fold_degradation import FoldSynthesizer, degrade, draw_fold, draw_fusion_crop, fold_table
from data.resident import AugFlags, ResidentImages, crop_u8, sample_table

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRID_CAP = 1024            # JITTER_GRID_CAP of csrc/jitter_kernels.hip: workgroups per launch, a lane takes a dword
GUARD = 512                # bytes / counts either side of lut and hist
SENTINEL_U8, SENTINEL_HIST, SENTINEL_F32, SENTINEL_COUNT = 0xAB, 0x5EADBEEF, 7.0, 123456


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "jitter.npz")))


@pytest.fixture(scope="module")
def lib():
    return sstem_native.load_library()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else np.asarray(a)


def _assert_same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), "%s: %d of %d elements differ, first at %s" % (what, int(bad.sum()), bad.size, np.argwhere(bad)[0])


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _lut_entry(lib, planes, codes, factors, shift=0):
    """sstem_jitter_lut_u8 inside guard bands, hist dirty on entry, the planes `shift` bytes past an aligned address.
    Returns (lut [n,256] uint8, hist [n,256] int64) as numpy, after checking that both bands are intact."""
    n, S_h, S_w = planes.shape
    store = torch.zeros((planes.size + 8,), dtype=torch.uint8, device=DEV)
    src = store[shift:shift + planes.size]
    src.copy_(_t(planes.reshape(-1)))
    assert src.data_ptr() % 4 == shift % 4
    lut = torch.full((2 * GUARD + n * 256,), SENTINEL_U8, dtype=torch.uint8, device=DEV)
    hist = torch.full((2 * GUARD + n * 256,), SENTINEL_HIST, dtype=torch.int32, device=DEV)
    code, factor = _t(np.asarray(codes, np.int32).reshape(n, J.OPS)), _t(np.asarray(factors, np.float32).reshape(n, J.OPS))
    rc = lib.sstem_jitter_lut_u8(src.data_ptr(), n, S_h, S_w, code.data_ptr(), factor.data_ptr(), lut.data_ptr() + GUARD,
                                 hist.data_ptr() + 4 * GUARD, _stream())
    sstem_native.check(rc, "jitter_lut")
    lut, hist = lut.cpu().numpy(), hist.cpu().numpy()
    for band in (lut[:GUARD], lut[GUARD + n * 256:]):
        assert (band == SENTINEL_U8).all(), "lut's guard band was written"
    for band in (hist[:GUARD], hist[GUARD + n * 256:]):
        assert (band == SENTINEL_HIST).all(), "hist's guard band was written"
    return lut[GUARD:GUARD + n * 256].reshape(n, 256), hist[GUARD:GUARD + n * 256].reshape(n, 256).astype(np.int64)


def _check_tables(lib, planes, steps, shift=0):
    codes, factors = J.step_arrays(steps)
    lut, hist = _lut_entry(lib, planes, codes, factors, shift)
    for i in range(planes.shape[0]):
        assert np.array_equal(hist[i], np.bincount(planes[i].reshape(-1), minlength=256)), "sample %d histogram" % i
        _assert_same(lut[i], J.lut_of(planes[i], steps[i]), "sample %d table" % i)
    return lut, hist


def _em_like(rng, n, H, W):
    """A narrow histogram around a per-sample level: many lanes of a wave land in one bin."""
    level = rng.integers(60, 200, size=(n, 1, 1))
    return np.clip(np.rint(rng.normal(level, 9.0, size=(n, H, W))), 0, 255).astype(np.uint8)


# ---- the table entry -------------------------------------------------------------------------------------------------------------------
def test_chains_equal_pil_and_the_restatement(lib, golden):
    """Fixture (b): every image under every chain, one launch per image with a sample per chain."""
    for name, img in J.images().items():
        planes = np.stack([img] * len(J.CHAINS))
        lut, _ = _check_tables(lib, planes, [list(c) for c in J.CHAINS])
        for ci in range(len(J.CHAINS)):
            _assert_same(lut[ci][img], golden["c%d_%s" % (ci, name)], "chain %d on %s" % (ci, name))


def test_blend_fixture_through_constant_samples(lib, golden):
    """Fixture (a): a constant plane of value d has mean d, so a single contrast step by f is the blend towards d; 256 samples per
    factor in one launch of 2048 samples (more than the table kernel's grid), on 3 x 5 planes (unaligned bases)."""
    nf = len(J.BLEND_FACTORS)
    planes = np.broadcast_to(np.tile(np.arange(256, dtype=np.uint8), nf)[:, None, None], (nf * 256, 3, 5)).copy()
    steps = [[(J.CONTRAST, f)] for f in J.BLEND_FACTORS for _ in range(256)]
    assert len(steps) > GRID_CAP
    codes, factors = J.step_arrays(steps)
    lut, hist = _lut_entry(lib, planes, codes, factors)
    _assert_same(lut.reshape(nf, 256, 256), golden["blend"], "blend table")
    assert (hist[np.arange(nf * 256), np.tile(np.arange(256), nf)] == 15).all() and hist.sum() == 15 * nf * 256


SHAPES = [(3, 1, 1, 0), (3, 1, 7, 1), (3, 7, 1, 2), (5, 3, 5, 0), (5, 3, 5, 3), (2, 255, 257, 0), (2, 255, 257, 1), (16, 400, 400, 0)]


@pytest.mark.parametrize("n,H,W,shift", SHAPES)
def test_shapes_and_alignments(lib, n, H, W, shift):
    rng = np.random.default_rng(n * 1000 + H + W + shift)
    planes = _em_like(rng, n, H, W) if H * W > 64 else rng.integers(0, 256, size=(n, H, W), dtype=np.uint8)
    steps = [list(J.CHAINS[(i + shift) % len(J.CHAINS)]) for i in range(n)]
    if H == 400:
        assert (H * W // 4 + 255) // 256 * n > GRID_CAP                        # the sample walk wraps
    _check_tables(lib, planes, steps, shift)


def test_grid_cap_wraps_both_stride_loops_and_a_bin_passes_2_20(lib):
    """n = 2 at 1040 x 1040: 1057 dword workgroups per sample against the cap of 1024, so the dword walk wraps and one row of
    workgroups takes both samples; the second image is constant, one bin of 1081600."""
    S = 1040
    assert (S * S // 4 + 255) // 256 > GRID_CAP
    rng = np.random.default_rng(1040)
    planes = np.stack([_em_like(rng, 1, S, S)[0], np.full((S, S), 93, dtype=np.uint8)])
    _, hist = _check_tables(lib, planes, [list(J.CHAINS[7]), list(J.CHAINS[2])])
    assert hist[1, 93] == S * S > 1 << 20 and hist[1].sum() == S * S


def test_two_runs_give_the_same_bits(lib):
    rng = np.random.default_rng(77)
    planes = _em_like(rng, 16, 400, 400)
    codes, factors = J.step_arrays([list(J.CHAINS[i % len(J.CHAINS)]) for i in range(16)])
    first = _lut_entry(lib, planes, codes, factors)
    second = _lut_entry(lib, planes, codes, factors)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])


def test_a_bad_op_code_costs_its_own_row_only(lib):
    rng = np.random.default_rng(5)
    planes = rng.integers(0, 256, size=(5, 9, 11), dtype=np.uint8)
    steps = [list(J.CHAINS[i]) for i in range(5)]
    codes, factors = J.step_arrays(steps)
    codes[1, 2], codes[3, 0] = 4, -1                       # one past the last code in a late step, a negative one in the first
    lut, hist = _lut_entry(lib, planes, codes, factors)
    for i in range(5):
        assert np.array_equal(hist[i], np.bincount(planes[i].reshape(-1), minlength=256))
        if i in (1, 3):
            assert (lut[i] == SENTINEL_U8).all(), "sample %d has a bad op code and must stay unwritten" % i
        else:
            _assert_same(lut[i], J.lut_of(planes[i], steps[i]), "sample %d" % i)


def test_non_finite_factors_store_zero_and_stay_in_bounds(lib):
    """Outside the contract: NaN and infinite factors give a table (0 where t is not finite), nothing else is touched."""
    planes = np.random.default_rng(6).integers(0, 256, size=(3, 8, 8), dtype=np.uint8)
    steps = [[(J.BRIGHTNESS, float("nan"))], [(J.CONTRAST, float("inf"))], [(J.BRIGHTNESS, float("-inf")), (J.CONTRAST, 1.1)]]
    with np.errstate(invalid="ignore"):
        _check_tables(lib, planes, steps)


def test_python_layer_makes_the_same_tables(lib):
    rng = np.random.default_rng(8)
    planes = rng.integers(0, 256, size=(6, 33, 61), dtype=np.uint8)
    steps = [J.draw_jitter(random.Random(i), 0.5, 0.5, 0.5) for i in range(5)] + [[]]
    lut = jitter_luts(_t(planes), steps)
    assert lut.is_cuda and lut.dtype == torch.uint8 and tuple(lut.shape) == (6, 256)
    for i in range(6):
        _assert_same(lut[i], J.lut_of(planes[i], steps[i]), "sample %d" % i)
    _assert_same(lut[5], np.arange(256, dtype=np.uint8), "no steps: the identity")
    with pytest.raises(ValueError):
        jitter_luts(_t(planes), steps[:3])
    with pytest.raises(ValueError):
        jitter_luts(_t(planes[:1]), [[(9, 1.0)]])


# ---- the degrade entry -----------------------------------------------------------------------------------------------------------------
OUTPUTS = ("deformed", "flow2", "im", "lb", "zero_count")


def _degrade(lib, clean, interp, rows, window, lut="old", slots=None, gt_line=False):
    """sstem_fold_degrade_u8 (lut == "old") or sstem_fold_degrade_lut_u8 (lut None or [slots,256]) into sentinel-filled tensors."""
    n, nslots = len(rows), clean.shape[0]
    _, _, h, w = window
    folds = _t(np.asarray(rows, dtype=np.float64).reshape(n, R.PARAMS))
    slot = None if slots is None else _t(np.asarray(slots, dtype=np.int32))
    out = {"deformed": torch.full((nslots, h, w), SENTINEL_U8, dtype=torch.uint8, device=DEV),
           "flow2": torch.full((nslots, 2, h, w), SENTINEL_F32, dtype=torch.float32, device=DEV),
           "im": torch.full((nslots, 6, h, w), SENTINEL_F32, dtype=torch.float32, device=DEV),
           "lb": torch.full((nslots, 1, h, w), SENTINEL_F32, dtype=torch.float32, device=DEV),
           "zero_count": torch.full((nslots,), SENTINEL_COUNT, dtype=torch.int32, device=DEV)}
    cl, it = _t(clean), _t(interp)
    ins = (cl.data_ptr(), it.data_ptr(), folds.data_ptr(), _ptr(slot), n, nslots, clean.shape[1], clean.shape[2], *window, 1 if gt_line else 0)
    outs = tuple(out[k].data_ptr() for k in OUTPUTS)
    if isinstance(lut, str):
        rc = lib.sstem_fold_degrade_u8(*ins, *outs, _stream())
    else:
        table = None if lut is None else _t(lut)
        rc = lib.sstem_fold_degrade_lut_u8(*ins, _ptr(table), *outs, _stream())
    sstem_native.check(rc, "fold_degrade")
    return {k: v.cpu().numpy() for k, v in out.items()}


FOLDS = [(0.0, 17.0, 5, 10, 0.05), (1.0, -3.0, 5, 10, 0.1), (-0.6, 35.0, 20, 80, 0.1)]


@pytest.mark.parametrize("gt_line", [False, True])
def test_null_and_identity_tables_are_the_old_entry(lib, gt_line):
    H, W, window = 40, 56, (4, 6, 30, 44)
    rows = [R.scalars(*f) for f in FOLDS]
    clean = np.stack([R.image(40 + i, H, W) for i in range(5)])
    interp = np.stack([R.image(50 + i, H, W) for i in range(5)])
    slots = [4, 0, 2]
    old = _degrade(lib, clean, interp, rows, window, "old", slots, gt_line)
    identity = np.tile(np.arange(256, dtype=np.uint8), (5, 1))
    for name, lut in (("NULL", None), ("identity", identity)):
        new = _degrade(lib, clean, interp, rows, window, lut, slots, gt_line)
        for key in OUTPUTS:
            _assert_same(new[key], old[key], "%s table, %s" % (name, key))
    assert (old["deformed"][1] == SENTINEL_U8).all() and old["zero_count"][3] == SENTINEL_COUNT


@pytest.mark.parametrize("gt_line", [False, True])
def test_degrade_through_a_table(lib, gt_line):
    """n = 3 samples into slots (4, 0, 2) of 5: deformed, im[:, :3], flow2 and zero_count are the OLD entry's on the host-jittered
    planes; lb is the old entry's on the planes themselves, zero where the jittered sample is black with gt_line; im[:, 3:] is interp's
    window; slots 1 and 3 keep the sentinels."""
    H, W, window = 40, 56, (4, 6, 30, 44)
    rows = [R.scalars(*f) for f in FOLDS]
    rng = np.random.default_rng(12)
    clean = _em_like(rng, 5, H, W)
    clean[0, 10:14, 20:30] = 0                             # black pixels of the image itself: the table moves them (brightness keeps 0, contrast does not)
    interp = np.stack([R.image(50 + i, H, W) for i in range(5)])
    slots = [4, 0, 2]
    steps = [list(J.CHAINS[s]) for s in range(5)]
    lut = np.stack([J.lut_of(clean[s], steps[s]) for s in range(5)])
    assert all((lut[s] != np.arange(256)).any() for s in slots)
    jittered = np.stack([lut[s][clean[s]] for s in range(5)])
    new = _degrade(lib, clean, interp, rows, window, lut, slots, gt_line)
    on_jittered = _degrade(lib, jittered, interp, rows, window, "old", slots, gt_line)
    on_clean = _degrade(lib, clean, interp, rows, window, "old", slots, False)
    for key in ("deformed", "flow2", "im", "zero_count"):
        _assert_same(new[key], on_jittered[key], key)
    want_lb = on_clean["lb"].copy()
    if gt_line:
        for s in slots:
            want_lb[s, 0][new["deformed"][s] == 0] = 0.0
    _assert_same(new["lb"], want_lb, "lb")
    _assert_same(new["im"][:, 3:], on_clean["im"][:, 3:], "im[:, 3:]")
    for i, s in enumerate(slots):                          # and the restatement, output by output
        want = J.degrade(clean[s], interp[s], rows[i], window, lut[s], gt_line)
        for key in ("deformed", "flow2", "im", "lb"):
            _assert_same(new[key][s], want[key], "slot %d %s vs jitter_ref" % (s, key))
        assert int(new["zero_count"][s]) == want["zero_count"]
    for s in (1, 3):
        assert (new["deformed"][s] == SENTINEL_U8).all() and int(new["zero_count"][s]) == SENTINEL_COUNT
        assert all((new[k][s] == SENTINEL_F32).all() for k in ("flow2", "im", "lb"))


def test_degrade_through_a_table_past_the_grid_cap(lib):
    """n = 2 at 1040 x 1040 (4225 pixel workgroups per sample against the fold grid's 4096): one row of workgroups stages the table of
    the first sample, then the second's."""
    S = 1040
    rows = [R.scalars(-0.6, 700.0, 20, 80, 0.1), R.scalars(1 / 3, 50.0, 9, 30, 0.031)]
    rng = np.random.default_rng(1041)
    clean = _em_like(rng, 2, S, S)
    lut = np.stack([J.lut_of(clean[s], J.CHAINS[s]) for s in range(2)])
    new = _degrade(lib, clean, clean, rows, (0, 0, S, S), lut)
    old = _degrade(lib, np.stack([lut[s][clean[s]] for s in range(2)]), clean, rows, (0, 0, S, S), "old")
    for key in ("deformed", "flow2", "im", "zero_count"):
        _assert_same(new[key], old[key], key)


def test_python_degrade_takes_the_table():
    H = W = 64
    window = (8, 8, 48, 48)
    clean = np.stack([R.image(400 + i, H, W) for i in range(3)])
    interp = np.stack([R.image(410 + i, H, W) for i in range(3)])
    steps = [list(J.CHAINS[i]) for i in range(3)]
    lut = jitter_luts(_t(clean), steps)
    out = degrade(_t(clean), _t(interp), fold_table(FOLDS, DEV), window, gt_line=True, lut=lut)
    assert out.launches == 1
    for i in range(3):
        want = J.degrade(clean[i], interp[i], R.scalars(*FOLDS[i]), window, J.lut_of(clean[i], steps[i]), True)
        for key in ("deformed", "im", "lb"):
            _assert_same(getattr(out, key)[i], want[key], "sample %d %s" % (i, key))
        assert int(out.zero_count[i]) == want["zero_count"]


def test_both_entries_replay_in_a_graph(lib):
    H = W = 64
    window = (8, 8, 48, 48)
    rng = np.random.default_rng(9)
    clean_np = _em_like(rng, 3, H, W)
    clean, interp = _t(clean_np), _t(np.stack([R.image(410 + i, H, W) for i in range(3)]))
    steps = [list(J.CHAINS[i]) for i in range(3)]
    codes, factors = J.step_arrays(steps)
    code, factor, folds = _t(codes), _t(factors), fold_table(FOLDS, DEV)
    lut = torch.empty((3, 256), dtype=torch.uint8, device=DEV)
    hist = torch.empty((3, 256), dtype=torch.int32, device=DEV)
    eager = degrade(clean, interp, folds, window, gt_line=True, lut=jitter_luts(clean, steps))
    want = {k: getattr(eager, k).clone() for k in ("deformed", "im", "lb", "zero_count")}

    def run(out):
        sstem_native.check(lib.sstem_jitter_lut_u8(clean.data_ptr(), 3, H, W, code.data_ptr(), factor.data_ptr(), lut.data_ptr(),
                                                   hist.data_ptr(), _stream()), "jitter_lut")
        return degrade(clean, interp, folds, window, gt_line=True, out=out, lut=lut)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = run(None)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(out)
    for _ in range(2):
        lut.fill_(3)
        hist.fill_(-5)
        for k in want:
            getattr(out, k).fill_(3)
        graph.replay()
        torch.cuda.synchronize()
        for k, v in want.items():
            got = getattr(out, k)
            assert torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got, v.view(torch.int32) if v.dtype == torch.float32 else v), k
        for i in range(3):
            _assert_same(lut[i], J.lut_of(clean_np[i], steps[i]), "replayed table %d" % i)


# ---- the batchers ------------------------------------------------------------------------------------------------------------------------
def _steps_array(steps):
    return np.array(steps, dtype=np.float64).reshape(len(steps), 2)


def test_batch_of_one_reproduces_the_provider(golden):
    """Fixture (c) through FoldSynthesizer.batch: the crop drawn and cut on the host, then jitter and folds -- tensors, steps, stream."""
    images = C.images_of(C.FUSION_IMAGES)
    shapes = [images[p[0]].shape for p in C.FUSION_PAIRS]
    synth = FoldSynthesizer(det_size=C.FUSION_DET, min_zero=100)
    for seed in J.PROVIDER_SEEDS:
        key = "p%d_" % seed
        rng = random.Random(seed)
        clean, interp = C.fusion_crops(images, C.FUSION_PAIRS, C.draw_sample(rng, C.FUSION_FLAGS, shapes, C.FUSION_CROP), C.FUSION_CROP)
        batch = synth.batch(_t(clean[None]), _t(interp[None]), rng, "image", bool(seed & 1), jitter=J.PROVIDER_JITTER)
        _assert_same(batch.im[0], golden[key + "im"], key + "im")
        _assert_same(batch.lb[0], golden[key + "lb"], key + "lb")
        assert np.array_equal(_steps_array(batch.jitter_steps[0]), golden[key + "steps"])
        assert batch.drawn == batch.rounds == batch.launches == int(golden[key + "drawn"])
        assert rng.random() == float(golden[key + "next"])
        _assert_same(batch.lut[0], J.lut_of(clean, batch.jitter_steps[0]), key + "lut")


def test_batch_resident_of_one_reproduces_the_provider(golden):
    resident = ResidentImages(C.images_of(C.FUSION_IMAGES), DEV)
    synth = FoldSynthesizer(det_size=C.FUSION_DET, min_zero=100)
    for seed in J.PROVIDER_SEEDS:
        key = "p%d_" % seed
        rng = random.Random(seed)
        batch = synth.batch_resident(resident, C.FUSION_PAIRS, rng, 1, C.FUSION_CROP[0], AugFlags(*C.FUSION_FLAGS), "image", bool(seed & 1),
                                     jitter=J.PROVIDER_JITTER)
        _assert_same(batch.im[0], golden[key + "im"], key + "im")
        _assert_same(batch.lb[0], golden[key + "lb"], key + "lb")
        assert np.array_equal(_steps_array(batch.jitter_steps[0]), golden[key + "steps"])
        assert rng.random() == float(golden[key + "next"])


def test_batch_resident_of_four_draws_crop_then_jitter_per_slot():
    images = C.images_of(C.FUSION_IMAGES)
    resident = ResidentImages(images, DEV)
    synth = FoldSynthesizer(det_size=C.FUSION_DET, min_zero=100)
    shapes = [images[p[0]].shape for p in C.FUSION_PAIRS]
    S, B = C.FUSION_CROP[0], 4
    off = (S - C.FUSION_DET) // 2
    batch = synth.batch_resident(resident, C.FUSION_PAIRS, random.Random(10), B, S, AugFlags(*C.FUSION_FLAGS), "image", True, jitter=(0.5, 0.5, 0.0))
    rng = random.Random(10)
    for b in range(B):
        draw = C.draw_sample(rng, C.FUSION_FLAGS, shapes, C.FUSION_CROP)
        steps = J.draw_jitter(rng, 0.5, 0.5, 0.0)
        assert batch.crops[b] == (draw[1], draw[2], C.orientation_code(*draw[3])) and batch.jitter_steps[b] == steps and len(steps) == 2
        clean, interp = C.fusion_crops(images, C.FUSION_PAIRS, draw, C.FUSION_CROP)
        want = J.degrade(clean, interp, R.scalars(*batch.folds[b]), (off, off, C.FUSION_DET, C.FUSION_DET), J.lut_of(clean, steps), True)
        assert want["zero_count"] >= 100
        for key in ("deformed", "im", "lb"):
            _assert_same(getattr(batch, key)[b], want[key], "slot %d %s" % (b, key))


def test_batch_resident_without_jitter_is_the_parent_s_path():
    """jitter=None: the crops, then the rounds through sstem_fold_degrade_u8, composed here call by call as the batcher did before it
    knew of jitter -- the same tensors, folds, launches and stream position, and no table."""
    images = C.images_of(C.FUSION_IMAGES)
    resident = ResidentImages(images, DEV)
    synth = FoldSynthesizer(det_size=C.FUSION_DET, min_zero=100)
    S, B = C.FUSION_CROP[0], 4
    flags = AugFlags(*C.FUSION_FLAGS)
    shapes = [resident.shapes[p[0]] for p in C.FUSION_PAIRS]
    for seed in (5, 10):
        rng = random.Random(seed)
        batch = synth.batch_resident(resident, C.FUSION_PAIRS, rng, B, S, flags, "image", True)
        assert batch.lut is None and batch.jitter_steps is None
        ref = random.Random(seed)
        samples, planes = [], []
        for _ in range(B):
            k, i, j, code = draw_fusion_crop(ref, flags, shapes, (S, S))
            samples.append((i, j, code))
            planes.append(C.FUSION_PAIRS[k])
        crops = crop_u8(resident, sample_table(samples, planes, DEV), S, S)
        out, pending, launches = None, list(range(B)), 0
        while pending:
            draws = [draw_fold(ref, S, S) for _ in pending]
            out = degrade(crops[0], crops[1], draws, synth.window(S), "image", True, None if len(pending) == B else pending, out)
            launches += 1
            counts = out.zero_count.cpu()
            pending = [s for s in pending if int(counts[s]) < 100]
        assert batch.launches == batch.rounds == launches and rng.random() == ref.random()
        for key in ("deformed", "im", "lb", "zero_count"):
            _assert_same(getattr(batch, key), getattr(out, key).cpu().numpy(), "seed %d %s" % (seed, key))
