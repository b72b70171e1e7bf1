"""Training crops on the GPU (include/sstem_batch.h and its Python layer), every comparison bit for bit (uint32 views of the fp32
outputs) against the numpy restatement tests/crop_ref.py, and the batchers against the reference providers' fixture
tests/golden/crop_batch.npz."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import crop_ref as C
import fold_ref as R
import sstem_native
from data.fold_degradation import FoldSynthesizer
from data.interp_batch import InterpBatcher
from data.resident import SP_ROTATION_FLIP, AugFlags, ResidentImages, crop_f32, crop_u8, sample_table
from data.sp_patches import SP_INVERT, SP_NAMES, SP_REVERSED, sp_patches

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRID_CAP = 4096            # BATCH_GRID_CAP of csrc/batch_kernels.hip: workgroups (tiles) per launch
SENTINEL = 0xAB
SENTINEL_F32 = 7.0


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "crop_batch.npz")))


@pytest.fixture(scope="module")
def lib():
    return sstem_native.load_library()


@pytest.fixture(scope="module")
def two_images():
    images = [C.image(11, 131, 140), C.image(12, 140, 131)]
    return images, ResidentImages(images, DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else np.asarray(a)


def _assert_same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), "%s: %d of %d elements differ, first at %s" % (what, int(bad.sum()), bad.size, np.argwhere(bad)[0])


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded_u8(lib, resident, table, S_h, S_w, guard):
    """sstem_crop_orient_u8 into a sentinel-filled buffer with `guard` sentinel bytes on either side (an odd guard also takes the
    output off dword alignment).  Returns the payload [P,n,S_h,S_w] as numpy after checking both guards."""
    size = table.P * table.n * S_h * S_w
    buf = torch.full((guard + size + guard,), SENTINEL, dtype=torch.uint8, device=DEV)
    rc = lib.sstem_crop_orient_u8(resident.pool.data_ptr(), resident.table.data_ptr(), len(resident), table.samples.data_ptr(),
                                  table.plane_image.data_ptr(), table.n, table.P, S_h, S_w, buf.data_ptr() + guard, _stream())
    sstem_native.check(rc, "crop_orient_u8")
    host = buf.cpu().numpy()
    assert (host[:guard] == SENTINEL).all() and (host[guard + size:] == SENTINEL).all(), "a guard byte was written"
    return host[guard:guard + size].reshape(table.P, table.n, S_h, S_w)


def _guarded_f32(lib, resident, table, S_h, S_w, chan, C0, invert=0, guard=33, skip_out1=False):
    """sstem_crop_orient_f32 into sentinel-filled buffers with guard floats around each output -> (out0, out1) as numpy."""
    C1 = len(chan) - C0
    outs, bufs = [], []
    for Cn in (C0, C1):
        size = table.n * Cn * S_h * S_w
        bufs.append((torch.full((guard + size + guard,), SENTINEL_F32, dtype=torch.float32, device=DEV), size, Cn))
    arr = (ctypes.c_int32 * len(chan))(*chan)
    p1 = None if (C1 == 0 or skip_out1) else bufs[1][0].data_ptr() + 4 * guard
    rc = lib.sstem_crop_orient_f32(resident.pool.data_ptr(), resident.table.data_ptr(), len(resident), table.samples.data_ptr(),
                                   table.plane_image.data_ptr(), table.n, table.P, S_h, S_w, arr, C0, C1, invert,
                                   bufs[0][0].data_ptr() + 4 * guard, p1, _stream())
    sstem_native.check(rc, "crop_orient_f32")
    for buf, size, Cn in bufs:
        host = buf.cpu().numpy()
        assert (host[:guard] == SENTINEL_F32).all() and (host[guard + size:] == SENTINEL_F32).all(), "a guard float was written"
        outs.append(host[guard:guard + size].reshape(table.n, Cn, S_h, S_w))
    return outs


def _origins(H, W, S_h, S_w):
    """The four corners and an odd interior origin (where the window leaves room for one)."""
    my, mx = H - S_h, W - S_w
    inner = (min(my, 1 if my < 3 else 3), min(mx, 1 if mx < 5 else 5))
    return sorted({(0, 0), (0, mx), (my, 0), (my, mx), inner})


@pytest.mark.parametrize("S", [1, 5, 37, 64, 65, 130])
def test_every_code_on_square_windows(lib, two_images, S):
    images, resident = two_images
    samples, planes = [], []
    for k, img in enumerate(images):
        for oy, ox in _origins(img.shape[0], img.shape[1], S, S):
            for code in range(8):
                samples.append((oy, ox, code))
                planes.append((k,))
    assert any(oy % 2 == 1 and ox % 2 == 1 for oy, ox, _ in samples)
    table = sample_table(samples, planes, DEV)
    want = C.crop_u8(images, samples, planes, S, S)
    for guard in (64, 61):
        _assert_same(_guarded_u8(lib, resident, table, S, S, guard), want, "u8, guard %d" % guard)
    out0, _ = _guarded_f32(lib, resident, table, S, S, [0], 1)
    _assert_same(out0, C.to_f32(want[0])[:, None], "f32")


@pytest.mark.parametrize("S_h,S_w", [(7, 1), (1, 7), (33, 61), (61, 33), (3, 130)])
def test_non_square_windows(lib, two_images, S_h, S_w):
    images, resident = two_images
    samples = [(oy, ox, code) for oy, ox in _origins(131, 131, S_h, S_w) for code in range(4)]
    planes = [(i % 2,) for i in range(len(samples))]
    table = sample_table(samples, planes, DEV)
    want = C.crop_u8(images, samples, planes, S_h, S_w)
    for guard in (64, 63):
        _assert_same(_guarded_u8(lib, resident, table, S_h, S_w, guard), want, "u8, guard %d" % guard)
    out0, _ = _guarded_f32(lib, resident, table, S_h, S_w, [0], 1)
    _assert_same(out0, C.to_f32(want[0])[:, None], "f32")


def test_mixed_sizes_and_planes_from_different_images(lib):
    shapes = [(96, 80), (64, 72), (70, 70), (131, 67), (66, 200)]
    images = [C.image(20 + i, h, w) for i, (h, w) in enumerate(shapes)]
    resident = ResidentImages(images, DEV)
    assert resident.nbytes == sum(h * w for h, w in shapes) and resident.table.cpu().tolist()[1] == [96 * 80, 64, 72]
    rng = random.Random(7)
    samples, planes = [], []
    for _ in range(24):
        ids = [rng.randrange(len(images)) for _ in range(3)]
        h, w = min(shapes[k][0] for k in ids), min(shapes[k][1] for k in ids)
        samples.append((rng.randint(0, h - 61), rng.randint(0, w - 61), rng.randrange(8)))
        planes.append(ids)
    assert any(len(set(ids)) == 3 for ids in planes)
    table = sample_table(samples, planes, DEV)
    _assert_same(crop_u8(resident, table, 61, 61), C.crop_u8(images, samples, planes, 61, 61), "u8")
    im, lb = crop_f32(resident, table, 61, 61, [0, 0, 0, 2, 2, 2, 1], 6)
    want = C.crop_f32(images, samples, planes, 61, 61, [0, 0, 0, 2, 2, 2, 1], 6)
    _assert_same(im, want[0], "im")
    _assert_same(lb, want[1], "lb")


def test_bad_samples_write_nothing(lib, two_images):
    """Bad id, bad code, a window one pixel outside (each side, and in the second plane's smaller image only), a transposing code on a
    non-square window: sentinels stay, guards stay, the good neighbours are written."""
    images, resident = two_images
    for (S_h, S_w), rows in (((40, 40), [((0, 0, 5), (0, 1)), ((0, 0, 0), (0, 2)), ((0, 0, 0), (-1, 1)), ((3, 3, 8), (0, 1)), ((3, 3, -1), (0, 1)),
                                        ((92, 0, 0), (0, 0)), ((0, 101, 0), (0, 0)), ((-1, 0, 0), (0, 0)), ((0, -1, 0), (0, 0)),
                                        ((91, 100, 7), (0, 0)), ((95, 0, 0), (1, 0)), ((0, 95, 0), (0, 1)), ((91, 91, 6), (1, 0))]),
                             ((20, 40), [((0, 0, 4), (0, 1)), ((0, 0, 7), (0, 1)), ((0, 0, 3), (0, 1)), ((111, 91, 2), (0, 1)), ((112, 91, 2), (0, 1))])):
        samples, planes = [r[0] for r in rows], [r[1] for r in rows]
        writes = [C.sample_writes(images, ids, s[0], s[1], s[2], S_h, S_w) for s, ids in zip(samples, planes)]
        assert any(writes) and not all(writes)
        table = sample_table(samples, planes, DEV)
        want = C.crop_u8(images, samples, planes, S_h, S_w, out=np.full((2, len(rows), S_h, S_w), SENTINEL, np.uint8))
        got = _guarded_u8(lib, resident, table, S_h, S_w, 61)
        _assert_same(got, want, "u8 %dx%d" % (S_h, S_w))
        for i, w in enumerate(writes):
            assert w or (got[:, i] == SENTINEL).all()
        chan = [0, 1, 1, 0]
        w0, w1 = C.crop_f32(images, samples, planes, S_h, S_w, chan, 3, out0=np.full((len(rows), 3, S_h, S_w), SENTINEL_F32, np.float32),
                            out1=np.full((len(rows), 1, S_h, S_w), SENTINEL_F32, np.float32))
        out0, out1 = _guarded_f32(lib, resident, table, S_h, S_w, chan, 3)
        _assert_same(out0, w0, "f32 out0")
        _assert_same(out1, w1, "f32 out1")


def test_f32_channel_maps(lib, two_images):
    images, resident = two_images
    third = [C.image(13, 135, 135)]
    images = images + third
    resident = ResidentImages(images, DEV)
    samples = [(1, 3, code) for code in range(8)] + [(60, 59, 6)]
    planes = [(i % 3, (i + 1) % 3, (i + 2) % 3) for i in range(len(samples))]
    table = sample_table(samples, planes, DEV)
    S = 70
    u8 = C.crop_u8(images, samples, planes, S, S)
    # the IFNet map: replicated channels identical, bits of float32(b) / float32(255)
    chan = [0, 0, 0, 2, 2, 2, 1]
    im, lb = _guarded_f32(lib, resident, table, S, S, chan, 6)
    f255 = np.float32(255)
    for c, p in enumerate(chan[:6]):
        _assert_same(im[:, c], u8[p].astype(np.float32) / f255, "im channel %d" % c)
    _assert_same(lb[:, 0], u8[1].astype(np.float32) / f255, "lb")
    assert np.array_equal(_bits(im[:, 0]), _bits(im[:, 1])) and np.array_equal(_bits(im[:, 3]), _bits(im[:, 5]))
    # every byte value goes through the division
    assert set(np.unique(u8[0])) == set(range(256))
    # out1 NULL with C1 == 0; a plane no channel reads
    only, none = _guarded_f32(lib, resident, table, S, S, [2, 0], 2)
    assert none.size == 0
    _assert_same(only, np.stack([C.to_f32(u8[2]), C.to_f32(u8[0])], axis=1), "C1 == 0")
    # inverted channels
    inv, inv1 = _guarded_f32(lib, resident, table, S, S, [0, 0, 1, 1], 2, invert=0b1010)
    _assert_same(inv[:, 0], C.to_f32(u8[0]), "plain")
    _assert_same(inv[:, 1], C.to_f32(255 - u8[0]), "inverted")
    _assert_same(inv1[:, 0], C.to_f32(u8[1]), "plain, out1")
    _assert_same(inv1[:, 1], C.to_f32(255 - u8[1]), "inverted, out1")
    want = C.crop_f32(images, samples, planes, S, S, [0, 0, 1, 1], 2, invert=0b1010)
    _assert_same(inv, want[0], "crop_ref out0")
    _assert_same(inv1, want[1], "crop_ref out1")


def test_fourteen_channels_and_sp_patches():
    imgs = [C.image(40 + i, 90, 84) for i in range(20)]
    resident = ResidentImages(imgs, DEV)
    rng = random.Random(3)
    B, S = 9, 66
    ids14, origin, case = [], [], []
    for b in range(B):
        ids = [rng.randrange(20) for _ in range(14)]
        for c in SP_REVERSED:
            ids[c] = None
        ids14.append(ids)
        origin.append((rng.randint(0, 90 - S), rng.randint(0, 84 - S)))
        case.append(b % 8)
    got = sp_patches(resident, ids14, origin, case, S)
    assert list(got) == list(SP_NAMES) and len(got) == 14
    planes = [[ids[SP_REVERSED.get(c, c)] for c in range(14)] for ids in ids14]
    samples = [(oy, ox, SP_ROTATION_FLIP[a]) for (oy, ox), a in zip(origin, case)]
    want, _ = C.crop_f32(imgs, samples, planes, S, S, list(range(14)), 14, invert=SP_INVERT)
    for c, name in enumerate(SP_NAMES):
        assert tuple(got[name].shape) == (B, 1, S, S)
        _assert_same(got[name].contiguous(), want[:, c:c + 1], name)
    # the dataset's own words for one sample: RotationFlip of the crop, and 255 - mask for a reversed one
    b, c = 3, 8
    crop = imgs[ids14[b][SP_REVERSED[c]]][origin[b][0]:origin[b][0] + S, origin[b][1]:origin[b][1] + S]
    rot = np.fliplr(np.rot90(crop, 1))                     # case 3
    assert case[b] == 3
    _assert_same(got[SP_NAMES[c]][b, 0].contiguous(), (255 - rot).astype(np.float32) / np.float32(255), "reversed mask")


def test_grid_stride_wraps(lib):
    """5000 samples of 5 x 5 against the cap of 4096 workgroups, and 2 planes of 1040 x 1040 (17 x 17 tiles each)."""
    images = [C.image(60, 1100, 1090), C.image(61, 1090, 1100)]
    resident = ResidentImages(images, DEV)
    rng = random.Random(11)
    n = 5000
    assert n > GRID_CAP
    samples = [(rng.randint(0, 1085), rng.randint(0, 1085), rng.randrange(8)) for _ in range(n)]
    planes = [(rng.randrange(2),) for _ in range(n)]
    table = sample_table(samples, planes, DEV)
    want = C.crop_u8(images, samples, planes, 5, 5)
    _assert_same(_guarded_u8(lib, resident, table, 5, 5, 61), want, "5000 x 5 x 5 u8")
    out0, _ = _guarded_f32(lib, resident, table, 5, 5, [0], 1)
    _assert_same(out0, C.to_f32(want[0])[:, None], "5000 x 5 x 5 f32")
    for code in (0, 5):
        samples, planes = [(33, 27, code)], [(0, 1)]
        table = sample_table(samples, planes, DEV)
        want = C.crop_u8(images, samples, planes, 1040, 1040)
        _assert_same(crop_u8(resident, table, 1040, 1040), want, "1040 u8 code %d" % code)
        out0, _ = crop_f32(resident, table, 1040, 1040, [1, 0], 2)
        _assert_same(out0[0, 0], C.to_f32(want[1, 0]), "1040 f32 code %d" % code)


# ---- the batchers ------------------------------------------------------------------------------------------------------------------------
def test_interp_batcher_equals_the_reference(golden):
    images = C.images_of(C.INTERP_IMAGES)
    resident = ResidentImages(images, DEV)
    for fname, flags in C.INTERP_FLAG_SETS.items():
        batcher = InterpBatcher(resident, C.INTERP_TRIPLETS, C.INTERP_CROP[0], AugFlags(*flags))
        for seed in C.INTERP_SEEDS if fname == "all" else C.INTERP_SEEDS[:C.INTERP_OTHER_SEEDS]:
            key = "i_%s_%d_" % (fname, seed)
            rng = random.Random(seed)
            im, lb = batcher.batch(rng, 1)
            _assert_same(im[0], golden[key + "im"], key + "im")
            _assert_same(lb[0], golden[key + "lb"], key + "lb")
            assert rng.random() == float(golden[key + "next"])
    # a batch of several: slot order, against the restatement
    batcher = InterpBatcher(resident, C.INTERP_TRIPLETS, C.INTERP_CROP[0], AugFlags(*C.ALL_FLAGS))
    im, lb = batcher.batch(random.Random(99), 5)
    rng = random.Random(99)
    shapes = [images[t[0]].shape for t in C.INTERP_TRIPLETS]
    for b in range(5):
        wi, wl = C.interp_sample(images, C.INTERP_TRIPLETS, C.draw_sample(rng, C.ALL_FLAGS, shapes, C.INTERP_CROP), C.INTERP_CROP)
        _assert_same(im[b], wi, "slot %d im" % b)
        _assert_same(lb[b], wl, "slot %d lb" % b)


def test_batch_resident_single_sample_equals_the_reference(golden):
    images = C.images_of(C.FUSION_IMAGES)
    resident = ResidentImages(images, DEV)
    synth = FoldSynthesizer(det_size=C.FUSION_DET, min_zero=100)
    for seed in C.FUSION_SEEDS:
        key = "f_%d_" % seed
        rng = random.Random(seed)
        batch = synth.batch_resident(resident, C.FUSION_PAIRS, rng, 1, C.FUSION_CROP[0], AugFlags(*C.FUSION_FLAGS), "image", bool(seed & 1))
        _assert_same(batch.im[0], golden[key + "im"], key + "im")
        _assert_same(batch.lb[0], golden[key + "lb"], key + "lb")
        assert rng.random() == float(golden[key + "next"])


def test_batch_resident_of_four_equals_crop_ref_then_fold_ref():
    images = C.images_of(C.FUSION_IMAGES)
    resident = ResidentImages(images, DEV)
    synth = FoldSynthesizer(det_size=C.FUSION_DET, min_zero=100)
    shapes = [images[p[0]].shape for p in C.FUSION_PAIRS]
    S, B = C.FUSION_CROP[0], 4
    off = (S - C.FUSION_DET) // 2
    for seed in (5, 10):
        batch = synth.batch_resident(resident, C.FUSION_PAIRS, random.Random(seed), B, S, AugFlags(*C.FUSION_FLAGS), "image", True)
        rng = random.Random(seed)
        draws = [C.draw_sample(rng, C.FUSION_FLAGS, shapes, C.FUSION_CROP) for _ in range(B)]        # all crop draws first, in slot order
        assert batch.crops == [(d[1], d[2], C.orientation_code(*d[3])) for d in draws]
        for b in range(B):
            clean, interp = C.fusion_crops(images, C.FUSION_PAIRS, draws[b], C.FUSION_CROP)
            want = R.degrade(clean, interp, R.scalars(*batch.folds[b]), (off, off, C.FUSION_DET, C.FUSION_DET), True)
            assert want["zero_count"] >= 100
            for key in ("deformed", "im", "lb"):
                _assert_same(getattr(batch, key)[b], want[key], "seed %d slot %d %s" % (seed, b, key))


def test_crop_replays_in_a_graph():
    images = C.images_of(C.INTERP_IMAGES)
    resident = ResidentImages(images, DEV)
    samples, planes = [(3, 5, 6), (0, 0, 1)], [(0, 1, 2), (4, 5, 6)]
    table = sample_table(samples, planes, DEV)
    want = C.crop_f32(images, samples, planes, 40, 40, [0, 0, 0, 2, 2, 2, 1], 6)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        im, lb = crop_f32(resident, table, 40, 40, [0, 0, 0, 2, 2, 2, 1], 6)
        u8 = crop_u8(resident, table, 40, 40)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        crop_f32(resident, table, 40, 40, [0, 0, 0, 2, 2, 2, 1], 6, 0, im, lb)
        crop_u8(resident, table, 40, 40, u8)
    for _ in range(2):
        im.fill_(3), lb.fill_(3), u8.fill_(3)
        graph.replay()
        torch.cuda.synchronize()
        _assert_same(im, want[0], "im")
        _assert_same(lb, want[1], "lb")
        _assert_same(u8, C.crop_u8(images, samples, planes, 40, 40), "u8")
