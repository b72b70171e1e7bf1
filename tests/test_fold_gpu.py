"""Fold synthesis on the GPU (include/sstem_fold.h and its Python layer), every comparison bit for bit (uint32 views of the fp32
outputs): against the reference's fixture tests/golden/fold.npz with the doubles recorded there, and against the numpy restatement
tests/fold_ref.py with doubles derived on this host, so that a libm difference between machines cannot matter."""
import os
import random

import numpy as np
import pytest
import torch

import fold_ref as R
import sstem_native
from data.fold_degradation import FoldSynthesizer, degrade, fold_table
from utils.flow_synthesis import fold_scalars, gen_flow
from utils.image_warp import image_warp

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRID_CAP = 4096            # FOLD_GRID_CAP of csrc/fold_kernels.hip: workgroups of 256 pixels per launch


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "fold.npz")))


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


def _fold_flow(lib, rows, H, W):
    n = len(rows)
    folds = _t(np.asarray(rows, dtype=np.float64).reshape(n, R.PARAMS))
    flow = torch.full((n, H, W, 2), 7.0, dtype=torch.float32, device=DEV)
    flow2 = torch.full_like(flow, 7.0)
    mask = torch.full((n, H, W), 9, dtype=torch.uint8, device=DEV)
    sstem_native.check(lib.sstem_fold_flow(folds.data_ptr(), n, H, W, flow.data_ptr(), flow2.data_ptr(), mask.data_ptr(), _stream()), "fold_flow")
    return flow, flow2, mask


SENTINEL_U8, SENTINEL_F32, SENTINEL_COUNT = 0xAB, 7.0, 123456


def _degrade(lib, clean, interp, rows, window, slots=None, nslots=None, gt_line=False, skip=()):
    """sstem_fold_degrade_u8 into sentinel-filled tensors; `skip` names the outputs passed as NULL.  Returns the dict of tensors."""
    n = len(rows)
    nslots = clean.shape[0] if nslots is None else nslots
    _, _, h, w = window
    folds = _t(np.asarray(rows, dtype=np.float64).reshape(n, R.PARAMS))
    slot = None if slots is None else _t(np.asarray(slots, dtype=np.int32))
    out = {"deformed": torch.full((nslots, h, w), SENTINEL_U8, dtype=torch.uint8, device=DEV),
           "flow2": torch.full((nslots, 2, h, w), SENTINEL_F32, dtype=torch.float32, device=DEV),
           "im": torch.full((nslots, 6, h, w), SENTINEL_F32, dtype=torch.float32, device=DEV),
           "lb": torch.full((nslots, 1, h, w), SENTINEL_F32, dtype=torch.float32, device=DEV),
           "zero_count": torch.full((nslots,), SENTINEL_COUNT, dtype=torch.int32, device=DEV)}
    p = {k: (None if k in skip else v.data_ptr()) for k, v in out.items()}
    cl, it = _t(clean), (None if interp is None else _t(interp))
    rc = lib.sstem_fold_degrade_u8(cl.data_ptr(), _ptr(it), folds.data_ptr(), _ptr(slot), n, nslots, clean.shape[1], clean.shape[2], *window,
                                   1 if gt_line else 0, p["deformed"], p["flow2"], p["im"], p["lb"], p["zero_count"], _stream())
    sstem_native.check(rc, "fold_degrade")
    return out


def _check_degrade(out, want, slot, what, keys=("deformed", "flow2", "im", "lb")):
    for key in keys:
        _assert_same(out[key][slot], want[key], "%s %s" % (what, key))
    assert int(out["zero_count"][slot]) == want["zero_count"] == int((want["deformed"] == 0).sum()), what


# host-derived folds for the comparisons with fold_ref: positive, negative and zero slope, a vertical line, exact ties
FOLDS = [(0.0, 17.0, 5, 10, 0.05), (1.0, -3.0, 5, 10, 0.1), (-0.6, 35.0, 20, 80, 0.1), R.gen_line([0, 10], [40, 10]) + (5, 10, 0.1),
         (1 / 3, 0.0, 6, 7, 0.031), (-1.0, 40.0, 6, 13, 0.00001)]


# ---- fixture (a): the recorded doubles, against the reference's arrays --------------------------------------------------------------
def test_fixture_flow_warp_and_deformed(lib, golden):
    for name in R.FOLD_CASES:
        H, W, _, img = R.fold_case(name)
        row = golden[name + "_row"]
        flow, flow2, mask = _fold_flow(lib, [row], H, W)
        _assert_same(flow[0], golden[name + "_flow"], name + " flow")
        _assert_same(flow2[0], golden[name + "_flow2"], name + " flow2")
        _assert_same(mask[0], golden[name + "_mask"], name + " mask")
        ref_flow = _t(golden[name + "_flow"])
        for mode in ("bilinear", "nearest"):
            _assert_same(image_warp(_t(img), ref_flow, mode), golden[name + "_warp_" + mode], "%s warp %s" % (name, mode))
        out = _degrade(lib, img[None], img[None], [row], (0, 0, H, W))
        _assert_same(out["deformed"][0], golden[name + "_deformed"], name + " deformed")
        _assert_same(out["flow2"][0], np.ascontiguousarray(np.transpose(golden[name + "_flow2"], (2, 0, 1))), name + " fused flow2")
        assert int(out["zero_count"][0]) == int((golden[name + "_deformed"] == 0).sum())


def test_gen_flow_of_the_python_layer(golden):
    """The reference's call, on this host's doubles -- against fold_ref, and against the fixture where the doubles agree."""
    for name in ("k0_ties", "k_plus1", "non_square"):
        H, W, fold, _ = R.fold_case(name)
        flow, flow2, mask = gen_flow(H, W, *fold)
        assert flow.is_cuda and mask.dtype == torch.float64 and tuple(mask.shape) == (H, W)
        want = R.flow(R.scalars(*fold), H, W)
        _assert_same(flow, want[0], name + " flow")
        _assert_same(flow2, want[1], name + " flow2")
        _assert_same(mask, want[2].astype(np.float64), name + " mask")
        if np.array_equal(R.scalars(*fold), golden[name + "_row"]):
            _assert_same(flow, golden[name + "_flow"], name + " flow vs fixture")


# ---- against fold_ref, doubles derived on this host ------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(40, 56), (33, 61), (1, 7), (7, 1)])
def test_flow_planes(lib, H, W):
    rows = [R.scalars(*f) for f in FOLDS]
    flow, flow2, mask = _fold_flow(lib, rows, H, W)
    for i, row in enumerate(rows):
        want = R.flow(row, H, W)
        _assert_same(flow[i], want[0], "fold %d flow" % i)
        _assert_same(flow2[i], want[1], "fold %d flow2" % i)
        _assert_same(mask[i], want[2], "fold %d mask" % i)


@pytest.mark.parametrize("H,W", [(40, 56), (33, 61), (1, 7), (7, 1)])
@pytest.mark.parametrize("C", [1, 3])
def test_warp_planes_and_channels(H, W, C):
    rng = np.random.default_rng(H * 100 + W + C)
    n = 2
    im = rng.integers(0, 256, size=(n, H, W, C), dtype=np.uint8)
    flows = np.stack([R.flow(R.scalars(*FOLDS[i + 1]), H, W)[0] for i in range(n)])
    for mode in ("bilinear", "nearest"):
        got = image_warp(_t(im), _t(flows), mode)
        for i in range(n):
            _assert_same(got[i], R.warp(im[i], flows[i], mode), "sample %d %s" % (i, mode))
    # the reference's shape conventions: [H,W,C] with [H,W,2], and [H,W] with [H,W,2]
    _assert_same(image_warp(_t(im[0]), _t(flows[0])), R.warp(im[0], flows[0]), "ndim 3")
    _assert_same(image_warp(_t(im[0, :, :, 0]), _t(flows[0])), R.warp(np.ascontiguousarray(im[0, :, :, 0]), flows[0]), "ndim 2")


def test_warp_every_clamp():
    """Flows of +-80 on a 40-pixel plane: every tap clamps on one side or the other, the weights come from the unclamped fraction."""
    rng = np.random.default_rng(80)
    H = W = 40
    im = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    fl = rng.uniform(-80, 80, size=(H, W, 2)).astype(np.float32)
    fl[0, :4] = [[-80, 80], [80, -80], [-0.0, 0.0], [39.5, -39.5]]
    x0 = np.arange(W)[None, :] + np.floor(fl[..., 0])
    y0 = np.arange(H)[:, None] + np.floor(fl[..., 1])
    assert (x0 < 0).any() and (x0 >= W - 1).any() and (y0 < 0).any() and (y0 >= H - 1).any() and ((x0 >= 0) & (x0 < W - 1)).any()
    for mode in ("bilinear", "nearest"):
        _assert_same(image_warp(_t(im), _t(fl), mode), R.warp(im, fl, mode), mode)


WINDOWS = {(40, 56): [(0, 0, 40, 56), (0, 9, 17, 30), (23, 9, 17, 30), (5, 0, 20, 11), (5, 45, 20, 11), (19, 27, 1, 1), (8, 8, 24, 40)],
           (33, 61): [(0, 0, 33, 61), (0, 0, 1, 61), (32, 60, 1, 1), (3, 7, 29, 47)]}


@pytest.mark.parametrize("H,W", list(WINDOWS))
@pytest.mark.parametrize("gt_line", [False, True])
def test_fused_outputs_on_windows(lib, H, W, gt_line):
    """The plane itself, a window on each edge, 1 x 1 and an inner window; n = 3 samples, each on its own image."""
    folds = FOLDS[:3] if H == 40 else FOLDS[3:]
    rows = [R.scalars(*f) for f in folds]
    clean = np.stack([R.image(20 + i, H, W) for i in range(3)])
    clean[0, 10:14, 20:30] = 0                             # black pixels of the image itself count too
    interp = np.stack([R.image(30 + i, H, W) for i in range(3)])
    for window in WINDOWS[(H, W)]:
        out = _degrade(lib, clean, interp, rows, window, gt_line=gt_line)
        for i in range(3):
            _check_degrade(out, R.degrade(clean[i], interp[i], rows[i], window, gt_line), i, "window %s sample %d" % (window, i))


def test_null_outputs_are_skipped(lib):
    H, W, window = 40, 56, (8, 8, 24, 40)
    row = R.scalars(*FOLDS[1])
    clean, interp = R.image(1, H, W)[None], R.image(2, H, W)[None]
    want = R.degrade(clean[0], interp[0], row, window)
    for skip in (("deformed",), ("flow2", "im"), ("lb", "zero_count"), ("deformed", "flow2", "im", "lb")):
        out = _degrade(lib, clean, None if "im" in skip else interp, [row], window, skip=skip)
        for key in ("deformed", "flow2", "im", "lb"):
            if key not in skip:
                _assert_same(out[key][0], want[key], "%s with %s skipped" % (key, skip))
        if "zero_count" not in skip:
            assert int(out["zero_count"][0]) == want["zero_count"]


def test_slots_write_only_the_named_samples(lib):
    """n = 3 launched samples into slots (4, 0, 2) of 5: each warps its slot's image; slots 1 and 3 keep the sentinels."""
    H, W, window = 40, 56, (4, 6, 30, 44)
    rows = [R.scalars(*f) for f in FOLDS[:3]]
    clean = np.stack([R.image(40 + i, H, W) for i in range(5)])
    interp = np.stack([R.image(50 + i, H, W) for i in range(5)])
    slots = [4, 0, 2]
    out = _degrade(lib, clean, interp, rows, window, slots=slots, gt_line=True)
    for i, s in enumerate(slots):
        _check_degrade(out, R.degrade(clean[s], interp[s], rows[i], window, True), s, "sample %d in slot %d" % (i, s))
    for s in (1, 3):
        assert (out["deformed"][s] == SENTINEL_U8).all() and int(out["zero_count"][s]) == SENTINEL_COUNT
        assert all((out[k][s] == SENTINEL_F32).all() for k in ("flow2", "im", "lb"))
    # a slot outside [0, slots) writes nothing
    out = _degrade(lib, clean, interp, rows, window, slots=[5, -1, 1])
    assert all(int(out["zero_count"][s]) == SENTINEL_COUNT for s in (0, 2, 3, 4)) and (out["deformed"][[0, 2, 3, 4]] == SENTINEL_U8).all()
    _check_degrade(out, R.degrade(clean[1], interp[1], rows[2], window), 1, "slot 1")


def test_im_is_the_u8_edge_of_deformed(lib):
    """im[:, 0:3] == sstem_gray_u8_to_f32(deformed), replicated; im[:, 3:6] the same of interp's window."""
    H, W, window = 33, 61, (3, 7, 29, 47)
    rows = [R.scalars(*f) for f in FOLDS[:2]]
    clean = np.stack([R.image(60 + i, H, W) for i in range(2)])
    interp = np.stack([R.image(70 + i, H, W) for i in range(2)])
    out = _degrade(lib, clean, interp, rows, window)
    npix = window[2] * window[3]
    for i in range(2):
        want = torch.empty((3, window[2], window[3]), dtype=torch.float32, device=DEV)
        sstem_native.check(lib.sstem_gray_u8_to_f32(out["deformed"][i].data_ptr(), want.data_ptr(), npix, 3, _stream()), "u8->f32")
        assert torch.equal(out["im"][i, 0:3].view(torch.int32), want.view(torch.int32))
        crop = _t(interp[i, 3:32, 7:54])
        sstem_native.check(lib.sstem_gray_u8_to_f32(crop.data_ptr(), want.data_ptr(), npix, 3, _stream()), "u8->f32")
        assert torch.equal(out["im"][i, 3:6].view(torch.int32), want.view(torch.int32))


def test_zero_count_is_overwritten_and_repeats():
    """The count over deformed, the same twice in a row into the same, never cleared, tensor (first filled with garbage)."""
    H, W = 64, 64
    clean = _t(np.stack([R.image(80 + i, H, W) for i in range(4)]))
    folds = fold_table(FOLDS[:4], DEV)
    out = degrade(clean, clean, folds, (8, 8, 48, 48))
    out.zero_count.fill_(-77777)
    counts = []
    for _ in range(3):
        degrade(clean, clean, folds, (8, 8, 48, 48), out=out)
        counts.append(out.zero_count.cpu().numpy().copy())
    want = (out.deformed == 0).sum(dim=(1, 2)).cpu().numpy()
    assert want.min() > 0
    for c in counts:
        assert np.array_equal(c, want)


def test_grid_cap_wraps_the_stride_loops(lib):
    """n = 2 at 1040 x 1040: 4225 pixel workgroups per sample against the cap, so the pixel walk wraps and one row of workgroups
    takes both samples."""
    S, n = 1040, 2
    assert (S * S + 255) // 256 > GRID_CAP
    rows = [R.scalars(-0.6, 700.0, 20, 80, 0.1), R.scalars(1 / 3, 50.0, 9, 30, 0.031)]
    clean = np.stack([R.image(90 + i, S, S) for i in range(n)])
    out = _degrade(lib, clean, None, rows, (0, 0, S, S), skip=("im",))
    flow, flow2, mask = _fold_flow(lib, rows, S, S)
    warped = image_warp(_t(clean[..., None]), flow, "bilinear")[..., 0] * mask          # both samples in one launch
    for i in range(n):
        want = R.degrade(clean[i], None, rows[i], (0, 0, S, S))
        _check_degrade(out, want, i, "sample %d" % i, keys=("deformed", "flow2", "lb"))
        _assert_same(flow2[i].permute(2, 0, 1).contiguous(), want["flow2"], "fold_flow flow2 %d" % i)
        _assert_same(warped[i], want["deformed"], "flow, warp, mask %d" % i)


# ---- the rejection loop ---------------------------------------------------------------------------------------------------------------
def test_synthesizer_single_sample_reproduces_the_reference(golden):
    clean = R.image(R.DEGRADE_IMAGE_SEED, R.DEGRADE_SIZE, R.DEGRADE_SIZE)
    synth = FoldSynthesizer(det_size=R.DEGRADE_SIZE - 2 * R.DEGRADE_OFFSET, min_zero=R.DEGRADE_MIN_ZERO)
    assert synth.window(R.DEGRADE_SIZE) == (8, 8, 48, 48)
    for seed in R.DEGRADE_SEEDS:
        batch = synth.batch(_t(clean[None]), _t(clean[None]), random.Random(seed), label="flow")
        key = "s%d_" % seed
        assert batch.drawn == batch.rounds == batch.launches == int(golden[key + "drawn"])
        _assert_same(batch.deformed[0], golden[key + "deformed"], "seed %d deformed" % seed)
        _assert_same(batch.lb[0], np.ascontiguousarray(np.transpose(golden[key + "flow2"], (2, 0, 1))), "seed %d flow label" % seed)


def test_synthesizer_batch_accepts_every_sample():
    B, S = 4, R.DEGRADE_SIZE
    clean = np.stack([R.image(200 + i, S, S) for i in range(B)])
    interp = np.stack([R.image(300 + i, S, S) for i in range(B)])
    synth = FoldSynthesizer(det_size=48, min_zero=R.DEGRADE_MIN_ZERO)
    redone = 0
    for seed in (10, 15, 1):                               # seeds whose first draws are rejected, and one more
        batch = synth.batch(_t(clean), _t(interp), random.Random(seed), label="image", gt_line=True)
        redone += batch.drawn - B
        assert batch.rounds == batch.launches >= 1 and batch.drawn >= B and tuple(batch.im.shape) == (B, 6, 48, 48)
        counts = batch.zero_count.cpu().numpy()
        assert (counts >= R.DEGRADE_MIN_ZERO).all()
        for i in range(B):
            want = R.degrade(clean[i], interp[i], R.scalars(*batch.folds[i]), (8, 8, 48, 48), True)
            assert np.array_equal(np.array(fold_scalars(*batch.folds[i])), R.scalars(*batch.folds[i]))
            for key in ("deformed", "im", "lb"):
                _assert_same(getattr(batch, key)[i], want[key], "seed %d sample %d %s" % (seed, i, key))
            assert counts[i] == want["zero_count"]
    assert redone > 0, "no seed exercised the redo of a rejected slot"


def test_degrade_replays_in_a_graph():
    H = W = 64
    window = (8, 8, 48, 48)
    clean = _t(np.stack([R.image(400 + i, H, W) for i in range(3)]))
    interp = _t(np.stack([R.image(410 + i, H, W) for i in range(3)]))
    folds = fold_table(FOLDS[:3], DEV)
    eager = degrade(clean, interp, folds, window, gt_line=True)
    want = {k: getattr(eager, k).clone() for k in ("deformed", "im", "lb", "zero_count")}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = degrade(clean, interp, folds, window, gt_line=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        degrade(clean, interp, folds, window, gt_line=True, out=out)
    for _ in range(2):
        for k in want:
            getattr(out, k).fill_(3)
        graph.replay()
        torch.cuda.synchronize()
        for k, v in want.items():
            got = getattr(out, k)
            assert torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got, v.view(torch.int32) if v.dtype == torch.float32 else v), k
