"""The flow colour code and the SFF image tail on the GPU (include/sstem_display.h and its Python layer), through the C-ABI.

The colour code is held to the numpy restatement tests/flow_color_ref.py, which tests/test_flow_color_cpu.py holds bit for bit to the
reference's recorded bytes: every byte must lie between the minimum and the maximum of the restatement over the 2k + 1 angle steps
(k = flow_color_ref.ATAN2_ULPS), so every byte that those steps do not move is held bit for bit, and the CPU file caps the others at
1e-3 of a case.  The tail entry has no transcendental and is held bit for bit to its restatement and to PIL's recorded bytes.
Outputs sit inside guard bands, the rgb base at 0, 1 and 2 bytes past a dword boundary; the workspace is never cleared: it starts
full of NaN flags and is dirtied by a larger call ahead of every case."""
import os

import numpy as np
import pytest
import torch

import flow_color_ref as R
import sstem_native

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRID_CAP = 4096            # DISPLAY_GRID_CAP of csrc/display_kernels.hip: workgroups per launch, a lane takes a pixel
PARTS = 128                # FLOW_MAXRAD_PARTS: workspace words per image
GUARD = 256                # bytes either side of every output, words either side of the workspace
SENTINEL_U8, SENTINEL_WS = 0xAB, 0x5EADBEEF
WS_IMAGES = 16             # images the tests' workspace serves
OK, NULL_POINTER, BAD_SHAPE, UNSUPPORTED = 0, 1, 2, 3

CASES = list(R.cases())
_ranges = {}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "flow_color.npz")))


@pytest.fixture(scope="module")
def lib():
    return sstem_native.load_library()


@pytest.fixture(scope="module")
def flows():
    return R.cases()


@pytest.fixture(scope="module")
def workspace(lib):
    """Between sentinel words, and never cleared: it starts as all ones, which every word reads as 'some radius was NaN'."""
    assert lib.sstem_flow_color_workspace_bytes(WS_IMAGES) == 4 * PARTS * WS_IMAGES
    ws = torch.full((2 * GUARD + PARTS * WS_IMAGES,), SENTINEL_WS, dtype=torch.int32, device=DEV)
    ws[GUARD:GUARD + PARTS * WS_IMAGES] = -1
    assert (ws.data_ptr() + 4 * GUARD) % 8 == 0
    return ws


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _range_of(key, flow_hw2):
    """(lo, hi, step0) of one image, computed once per key."""
    if key not in _ranges:
        _ranges[key] = R.byte_range(flow_hw2)
    return _ranges[key]


def _guarded(nbytes, offset=0):
    """A sentinel-filled uint8 buffer with `nbytes` between two guard bands, the payload `offset` bytes past a dword boundary."""
    buf = torch.full((2 * GUARD + nbytes + 4,), SENTINEL_U8, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 4 == 0 and GUARD % 4 == 0
    return buf, GUARD + offset


def _payload(buf, start, nbytes, what):
    host = buf.cpu().numpy()
    assert (host[:start] == SENTINEL_U8).all() and (host[start + nbytes:] == SENTINEL_U8).all(), "%s: a guard band was written" % what
    return host[start:start + nbytes]


def _workspace_bands_intact(ws, what):
    host = ws.cpu().numpy()
    assert (host[:GUARD] == SENTINEL_WS).all() and (host[GUARD + PARTS * WS_IMAGES:] == SENTINEL_WS).all(), "%s: the workspace's guard band was written" % what


def _colour(lib, ws, flow_dev, B, H, W, hwc, offset=0):
    """sstem_flow_color_u8 into a guarded buffer; returns uint8 [B,H,W,3] as numpy."""
    n = B * H * W * 3
    buf, start = _guarded(n, offset)
    assert (buf.data_ptr() + start) % 4 == offset
    rc = lib.sstem_flow_color_u8(flow_dev.data_ptr(), B, H, W, hwc, buf.data_ptr() + start, ws.data_ptr() + 4 * GUARD, _stream())
    sstem_native.check(rc, "sstem_flow_color_u8")
    got = _payload(buf, start, n, "rgb").reshape(B, H, W, 3)
    _workspace_bands_intact(ws, "flow colour")
    return got


def _dirty(lib, ws):
    """A larger call on the same workspace: more images and more partial maxima per image than any small case, every maximum above
    the cases' own, NaN flags in two images -- a launch that read a word its own call did not write would colour by it."""
    rng = np.random.default_rng(99)
    flow = (rng.standard_normal((WS_IMAGES, 2, 150, 140)) * np.logspace(4, 6.3, WS_IMAGES)[:, None, None, None]).astype(np.float32)
    flow[3, 0, 5, 5] = flow[WS_IMAGES - 1, 1, 0, 0] = np.nan
    _colour(lib, ws, _t(flow), WS_IMAGES, 150, 140, 0)


def _hold(got, key, flow_hw2, what):
    """Every byte inside the range over the angle steps; returns how many differ from step 0."""
    lo, hi, step0 = _range_of(key, flow_hw2)
    assert got.shape == step0.shape and got.dtype == np.uint8
    bad = (got < lo) | (got > hi)
    assert not bad.any(), "%s: %d of %d bytes outside the restatement's range, first at %s: got %s, range %s..%s" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], lo[bad][0], hi[bad][0])
    return int((got != step0).sum())


def _run_images(lib, ws, images, what, offsets=(0, 1, 2)):
    """images: list of (key, [H,W,2] float32) of one shape, as a batch, in both layouts and at every alignment of rgb."""
    B = len(images)
    H, W, _ = images[0][1].shape
    hwc = np.stack([im for _, im in images])
    chw = np.ascontiguousarray(hwc.transpose(0, 3, 1, 2))
    differ = 0
    first = None
    for layout, data in ((1, hwc), (0, chw)):
        dev = _t(data)
        before = dev.clone()
        for offset in offsets:
            got = _colour(lib, ws, dev, B, H, W, layout, offset)
            for i, (key, im) in enumerate(images):
                differ += _hold(got[i], key, im, "%s image %d layout %d offset %d" % (what, i, layout, offset))
            if first is None:
                first = got
            assert np.array_equal(got, first), "%s: layout %d offset %d gives other bytes than the first run" % (what, layout, offset)
        assert torch.equal(dev.view(torch.int32), before.view(torch.int32)), "%s: the entry wrote its flow" % what
    print("%s: %d bytes differ from the step-0 restatement over %d runs of %d bytes" % (what, differ, 2 * len(offsets), first.size))
    return first


# ---- the colour code -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_cases_lie_inside_the_restatements_range(lib, workspace, flows, golden, name):
    _dirty(lib, workspace)
    got = _run_images(lib, workspace, [(name, flows[name])], name)[0]
    lo, hi, _ = _range_of(name, flows[name])
    sure = lo == hi
    assert np.array_equal(got[sure], golden["rgb_" + name][sure])            # bit for bit the reference's bytes wherever the angle decides nothing


def test_every_image_of_a_batch_takes_its_own_maximum(lib, workspace, golden):
    batch = R.batch_case()
    images = [("batch%d" % i, np.ascontiguousarray(batch[i].transpose(1, 2, 0))) for i in range(4)]
    _dirty(lib, workspace)
    got = _run_images(lib, workspace, images, "batch")
    sure = np.stack([_range_of(k, im)[0] == _range_of(k, im)[1] for k, im in images])
    assert np.array_equal(got[sure], golden["rgb_batch"][sure])


def test_grid_stride_passes_the_cap_by_a_ragged_remainder(lib, workspace, flows):
    flow, index, base = R.grid_cap_case(GRID_CAP * 256)
    H, W, _ = flow.shape
    assert (H * W + 255) // 256 > GRID_CAP and (H * W - GRID_CAP * 256) % 256 != 0
    _ranges["grid_cap"] = R.gather_range(_range_of(base, flows[base]), index, H, W)
    _dirty(lib, workspace)
    _run_images(lib, workspace, [("grid_cap", flow)], "grid cap", offsets=(1,))


def test_more_images_than_rows_of_workgroups(lib, workspace, flows):
    """A row of workgroups per image while the cap allows: 725 x 725 takes 2054 workgroups, more than half the cap, so one row walks all
    three images, each with its own maximum, and the maxima come from 128 fat workgroups that take 16 pixels a lane."""
    S = 725
    assert GRID_CAP // ((S * S + 255) // 256) == 1 and (S * S + 2047) // 2048 > PARTS
    images = []
    for i, base in enumerate(("randn30", "one_nan", "smooth")):
        flow, index = R.tiled(flows[base], S, S)
        _ranges["walk%d" % i] = R.gather_range(_range_of(base, flows[base]), index, S, S)
        images.append(("walk%d" % i, flow))
    _dirty(lib, workspace)
    _run_images(lib, workspace, images, "three images under one row", offsets=(2,))


def test_empty_shapes_are_successful_no_ops(lib, workspace):
    buf, start = _guarded(64)
    flow = torch.zeros(64, dtype=torch.float32, device=DEV)
    for B, H, W in ((0, 4, 4), (2, 0, 4), (2, 4, 0)):
        assert lib.sstem_flow_color_u8(flow.data_ptr(), B, H, W, 0, buf.data_ptr() + start, workspace.data_ptr() + 4 * GUARD, _stream()) == OK
        assert lib.sstem_flow_color_u8(None, B, H, W, 1, None, None, _stream()) == OK
        assert lib.sstem_sff_outputs_u8(None, None, None, B, H, W, buf.data_ptr() + start, None, None, _stream()) == OK
    assert (buf.cpu().numpy() == SENTINEL_U8).all()
    _workspace_bands_intact(workspace, "empty shapes")


def test_refusals_return_their_status_without_a_launch(lib, workspace):
    """Every non-offending argument is a real device buffer, so a check that wrongly passed would still run inside bounds."""
    flow = torch.zeros(2 * 2 * 8 * 8, dtype=torch.float32, device=DEV)
    buf, start = _guarded(2 * 8 * 8 * 3)
    f, rgb, ws, s = flow.data_ptr(), buf.data_ptr() + start, workspace.data_ptr() + 4 * GUARD, _stream()
    colour = lib.sstem_flow_color_u8
    assert colour(f, -1, 8, 8, 0, rgb, ws, s) == BAD_SHAPE and colour(f, 2, -8, 8, 0, rgb, ws, s) == BAD_SHAPE
    assert colour(f, 2, 8, -8, 1, rgb, ws, s) == BAD_SHAPE and b"negative" in lib.sstem_last_error()
    assert colour(f, 1, 32769, 1, 0, rgb, ws, s) == UNSUPPORTED and colour(f, 1, 1, 32769, 0, rgb, ws, s) == UNSUPPORTED
    assert colour(f, (1 << 24) + 1, 1, 1, 0, rgb, ws, s) == UNSUPPORTED
    assert colour(None, 2, 8, 8, 0, rgb, ws, s) == NULL_POINTER and colour(f, 2, 8, 8, 0, None, ws, s) == NULL_POINTER
    assert colour(f, 2, 8, 8, 0, rgb, None, s) == NULL_POINTER
    assert colour(f, 2, 8, 8, 0, rgb, ws + 4, s) == UNSUPPORTED and b"8-byte" in lib.sstem_last_error()
    tail = lib.sstem_sff_outputs_u8
    pred, warped, interp = flow.data_ptr(), flow.data_ptr(), buf.data_ptr() + start
    assert tail(pred, warped, interp, -1, 4, 4, rgb, None, None, s) == BAD_SHAPE
    assert tail(pred, warped, interp, 1, 32769, 1, rgb, None, None, s) == UNSUPPORTED
    assert tail(None, warped, interp, 1, 4, 4, rgb, None, None, s) == NULL_POINTER and b"pred_u8 needs pred" in lib.sstem_last_error()
    assert tail(pred, None, interp, 1, 4, 4, None, rgb, None, s) == NULL_POINTER and tail(pred, None, interp, 1, 4, 4, None, None, rgb, s) == NULL_POINTER
    assert tail(pred, warped, None, 1, 4, 4, None, None, rgb, s) == NULL_POINTER
    assert tail(None, None, None, 1, 4, 4, None, None, None, s) == OK           # nothing asked for
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == SENTINEL_U8).all()
    _workspace_bands_intact(workspace, "refusals")


# ---- the image tail ------------------------------------------------------------------------------------------------------------------
def _tail_inputs(B, H, W, seed):
    """pred and warped that hit the conversion's edges and the L < 2 boundary from both sides, interp random."""
    rng = np.random.default_rng(seed)
    n = B * H * W
    f = np.float32
    edge = np.array([0.0, 1 / 255, 2 / 255, np.nextafter(f(1 / 255), f(0)), np.nextafter(f(2 / 255), f(0)), np.nextafter(f(2 / 255), f(1)), 1.0,
                     np.nextafter(f(1), f(0)), 256 / 255, 1.5, 3.7, -1e-9, -1 / 255, -0.5, -2.0, 1e-30, np.nan], dtype=np.float32)
    levels = (np.arange(256, dtype=np.float32) + np.float32(0.5)) / np.float32(255)           # all 256 grey levels after truncation
    pool = np.concatenate([edge, levels])
    pred = np.resize(pool, n).astype(np.float32)
    grey = np.resize(np.roll(pool, 7), n).astype(np.float32)
    warped = np.stack([grey, grey, grey], 0)                                                  # grey triples: L is the byte itself
    third = n // 3
    warped[:, :third] = rng.random((3, third), dtype=np.float32) * np.float32(0.03)           # three unequal channels around L = 2
    warped[:, third:2 * third] = rng.random((3, third), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)
    warped = np.ascontiguousarray(warped.reshape(3, B, H * W).transpose(1, 0, 2)).reshape(B, 3, H, W)
    interp = rng.integers(0, 256, size=(B, H, W), dtype=np.uint8)
    return pred.reshape(B, H, W), warped, interp


def _tail(lib, pred, warped, interp, want=(True, True, True), offset=0):
    B, H, W = interp.shape
    sizes = (B * H * W, B * H * W * 3, B * H * W)
    bufs = [_guarded(n, offset) if w else None for n, w in zip(sizes, want)]
    ptr = [None if b is None else b[0].data_ptr() + b[1] for b in bufs]
    p, w, i = _t(pred), _t(warped), _t(interp)
    rc = lib.sstem_sff_outputs_u8(p.data_ptr() if want[0] else None, w.data_ptr() if want[1] or want[2] else None,
                                  i.data_ptr() if want[2] else None, B, H, W, ptr[0], ptr[1], ptr[2], _stream())
    sstem_native.check(rc, "sstem_sff_outputs_u8")
    shapes = ((B, H, W), (B, H, W, 3), (B, H, W))
    return [None if b is None else _payload(b[0], b[1], n, "tail output").reshape(shape) for b, n, shape in zip(bufs, sizes, shapes)]


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (3, 37, 53), (1, 1025, 1025)])
def test_tail_is_bit_for_bit_alone_and_in_combination(lib, B, H, W):
    pred, warped, interp = _tail_inputs(B, H, W, B * H + W)
    with np.errstate(invalid="ignore"):
        ref = R.sff_outputs(pred, warped, interp)
    if H * W > 1:
        L = R.luminance(ref[1])
        assert (L == 0).any() and (L == 1).any() and (L == 2).any() and (L == 3).any() and (ref[2] != L).any() and (ref[2] == L).any()
        assert set(np.unique(ref[0])) == set(range(256))
    if H * W > GRID_CAP * 256:
        assert (H * W - GRID_CAP * 256) % 256 != 0                           # the stride loop wraps by a ragged remainder
    combos = [(True, True, True), (True, False, False), (False, True, False), (False, False, True), (True, False, True), (False, True, True)]
    for k, want in enumerate(combos):
        got = _tail(lib, pred, warped, interp, want, offset=k % 3)
        for g, r, w in zip(got, ref, want):
            assert (g is None) == (not w)
            if w:
                assert np.array_equal(g, r), "outputs %s: %d bytes differ" % (want, int((g != r).sum()))


def test_tail_luminance_equals_pils_recorded_bytes(lib, golden):
    """Bytes k -> the float (k + 0.5) / 255 -> the entry's own conversion -> k again, so the recorded triples reach the luminance."""
    triples = golden["triples"]
    n = len(triples)
    warped = ((triples.T.astype(np.float32) + np.float32(0.5)) / np.float32(255)).reshape(1, 3, 1, n)
    assert np.array_equal(R.to_u8(warped).reshape(3, n).T, triples)
    interp = np.full((1, 1, n), 77, dtype=np.uint8)
    _, rgb, stitch = _tail(lib, np.zeros((1, 1, n), np.float32), warped, interp, (False, True, True))
    assert np.array_equal(rgb.reshape(n, 3), triples)
    L = golden["triples_L"]
    assert np.array_equal(stitch.reshape(n), np.where(L < 2, 77, L).astype(np.uint8))
    assert (L[:256] == np.arange(256)).all() and (stitch.reshape(n)[:2] == 77).all() and stitch.reshape(n)[2] == 2       # the boundary, both sides


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------
def test_python_layer_equals_the_entries(lib, workspace, flows):
    import sff_pipeline
    from utils.flow_display import dense_flow, flow_color_batch, flow_to_image
    flow = flows["smooth_noise"]
    want = _colour(lib, workspace, _t(flow), 1, R.H0, R.W0, 1)[0]
    one = dense_flow(_t(flow))
    assert one.is_cuda and one.dtype == torch.uint8 and tuple(one.shape) == (R.H0, R.W0, 3)
    assert np.array_equal(one.cpu().numpy(), want) and torch.equal(flow_to_image(_t(flow)), one)
    batch = _t(R.batch_case())
    both = flow_color_batch(batch)
    assert tuple(both.shape) == (4, R.H0, R.W0, 3)
    for i in range(4):
        assert torch.equal(dense_flow(batch[i].permute(1, 2, 0)), both[i])               # the permuted view is made contiguous, not reinterpreted
    assert torch.equal(flow_color_batch(_t(flow.transpose(2, 0, 1)[None]))[0], one)

    pred, warped, interp = _tail_inputs(2, 19, 23, 5)
    with np.errstate(invalid="ignore"):
        ref = R.sff_outputs(pred, warped, interp)
    out = sff_pipeline.outputs(_t(pred)[:, None], _t(warped), _t(interp))
    assert len(out) == 3 and all(np.array_equal(o.cpu().numpy(), r) for o, r in zip(out, ref))
    out = sff_pipeline.outputs(_t(pred), _t(warped), _t(interp)[:, None], flow=batch[:2, :, :19, :23])
    assert len(out) == 4 and all(np.array_equal(o.cpu().numpy(), r) for o, r in zip(out[:3], ref))
    assert torch.equal(out[3], flow_color_batch(batch[:2, :, :19, :23].contiguous()))


def test_python_layer_refuses_cpu_tensors_and_wrong_shapes():
    import sff_pipeline
    from utils.flow_display import dense_flow, flow_color_batch
    with pytest.raises(NotImplementedError):
        dense_flow(torch.zeros(4, 4, 2))
    with pytest.raises(NotImplementedError):
        flow_color_batch(np.zeros((1, 2, 4, 4), np.float32))
    with pytest.raises(NotImplementedError):
        sff_pipeline.outputs(torch.zeros(1, 4, 4), torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError):
        dense_flow(torch.zeros(2, 4, 4, device=DEV))
    with pytest.raises(TypeError):
        flow_color_batch(torch.zeros(1, 2, 4, 4, device=DEV, dtype=torch.float64))


def test_graph_capture_replays_to_the_same_bytes(flows):
    from utils.flow_display import flow_color_batch
    flow = _t(R.batch_case())
    eager = flow_color_batch(flow)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        flow_color_batch(flow)                           # this stream's workspace exists before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = flow_color_batch(flow)
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
