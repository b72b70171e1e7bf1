"""Every amax bound held to its tensor, through the C-ABI (include/sstem_conv.h, "Amax words and the scaled forward").

Producers: ONE element of known magnitude V is planted where a reduction can leave it out (tests/amax_cases.py: plane corners, the
last pixel of the last image, the ragged right / bottom tile, the second tile, the last channel of a ragged channel block) and the
word that comes back must say |V stored| exactly, with every other slot at 0 or |V stored|.  The maximum is made by the convolution
(a centre-tap one-hot weight, an input that is zero but for one element; V is a power of two, exact under every id) or by the
epilogue (bias, shift, residual).  sstem_amax_f32, the pre-pass of every tensor no producer bounded, is held on its own: every loop's
first and last element, unaligned pointers, the grid stride, guard bands around the tensor.  The fp16 weight packing is held in its
per-layer and its group form.  Consumers: a bound that lives in one chosen slot, at a binade's edge, at the clamps of
amax_exponent (csrc/conv_split_common.h) or above the true maximum must not change what the launch computes beyond the id's
tolerance (tests/test_conv_split_gpu.py ``_close``).

The launch helper, the restated dispatch rules and the instance rows are those of tests/test_conv_exact_gpu.py."""
import ctypes

import pytest
import torch

import amax_cases as AC
import conv_exact as CE
import hipnn.functional as HF
import sstem_native
import test_conv_exact_gpu as X
from test_conv_split_gpu import _close

pytestmark = pytest.mark.gpu

V = 2.0 ** 5
SIGNS = (1.0, -1.0)
F16 = HF.ALGO_MFMA_F16X3


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in ("SSTEM_SPLIT_WALK", "SSTEM_SPLIT_WALK_MIN_WGS", "SSTEM_SPLIT_WALK_CT", "SSTEM_WGRAD_PINGPONG"):
        monkeypatch.delenv(k, raising=False)
    yield
    HF.set_algorithm(HF.ALGO_AUTO)


def _p(t):
    return None if t is None else t.data_ptr()


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def _smallest_rows():
    """The smallest shape of each instance row of tests/test_conv_exact_gpu.py (rows that name the same instance share one)."""
    best = {}
    for name, shape, inst in X.FWD_ROWS:
        if inst not in best or _numel(shape) < _numel(best[inst][1]):
            best[inst] = (name, shape, inst)
    return list(best.values())


ROWS = _smallest_rows()
assert {r[2] for r in ROWS} == {r[2] for r in X.FWD_ROWS} and any(r[2][4] > 1 for r in ROWS)      # (a split-K row is among them)


# ---- sstem_amax_f32 --------------------------------------------------------------------------------------------------------------------
SWEEP = 4 * 256 * 1024                 # elements one pass of the capped grid covers: 1024 workgroups x 256 lanes x 4 floats
AMAX_NS = (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, SWEEP - 1, SWEEP + 1, 3 * SWEEP + 1029)
BAND = 64                              # floats of guard band on either side


def _amax_plants(n, off):
    """Indices worth planting at: 0, the last four, the first element of the tail loop (aligned: n - n % 4), the first element of the
    second workgroup and of the second and last grid-stride pass."""
    s = {0, n - 1, n - 2, n - 3, n - 4, n - n % 4, 1024, SWEEP, SWEEP + 1, (n // SWEEP) * SWEEP, 262144, 262145}
    if n <= 5:
        s |= set(range(n))
    return sorted(i for i in s if 0 <= i < n)


def _amax_runs(lib, n, off, plants):
    """One launch per (index, value) on a zero tensor of n floats that starts `off` floats behind a 16-byte boundary, between guard
    bands of 3e38; returns the words [len(plants), 1024] after ONE synchronisation."""
    buf = torch.full((BAND + off + n + BAND + 4,), AC.GUARD, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[BAND + off:BAND + off + n]
    t.zero_()
    words = torch.zeros(len(plants), AC.SLOTS, device="cuda")
    for k, (i, v) in enumerate(plants):
        t[i] = v
        assert lib.sstem_amax_f32(t.data_ptr(), n, words[k].data_ptr(), None) == 0
        t[i] = 0.0
    torch.cuda.synchronize()
    return words.cpu()


@pytest.mark.parametrize("n", AMAX_NS)
def test_amax_f32_finds_a_planted_element_anywhere(n):
    lib = X._lib()
    for off in range(4):
        plants = [(i, V if (i + off) % 2 else -V) for i in _amax_plants(n, off)]
        words = _amax_runs(lib, n, off, plants)
        for (i, v), w in zip(plants, words):
            AC.assert_word(w, abs(v), "n=%d, pointer offset %d floats, element %d = %r" % (n, off, i, v))


def test_amax_f32_special_values_and_the_nan_rule():
    """Negative, subnormal, -0.0 and inf; and a NaN beside a finite maximum.  The NaN rule, read from amax_kernel: the reduction is
    fmaxf(m, fabsf(x)), which returns its other operand for a NaN, and the slots are raised by an integer atomic max of non-negative
    floats' bit patterns -- a NaN is SKIPPED, the word holds the largest magnitude among the other elements (0 if there are none)."""
    lib = X._lib()
    nan, inf, sub = float("nan"), float("inf"), 2.0 ** -140
    for n, off in ((1025, 0), (1025, 1), (7, 3), (4, 0)):
        last = n - 1
        cases = [([(0, -3.0)], 3.0), ([(last, sub)], sub), ([(last, -sub)], sub), ([(0, -0.0), (last, -0.0)], 0.0),
                 ([(last, inf)], inf), ([(0, -inf), (last, 5.0)], inf),
                 ([(0, nan), (last, 5.0)], 5.0), ([(0, 5.0), (last, nan)], 5.0), ([(1, nan), (2, -7.0), (3, nan)], 7.0),
                 ([(0, nan)], 0.0), ([(last, nan)], 0.0)]
        buf = torch.full((BAND + off + n + BAND + 4,), AC.GUARD, device="cuda")
        t = buf[BAND + off:BAND + off + n]
        words = torch.zeros(len(cases), AC.SLOTS, device="cuda")
        for k, (plants, _) in enumerate(cases):
            t.zero_()
            for i, v in plants:
                t[i] = v
            assert lib.sstem_amax_f32(t.data_ptr(), n, words[k].data_ptr(), None) == 0
        torch.cuda.synchronize()
        for (plants, want), w in zip(cases, words.cpu()):
            AC.assert_word(w, want, "n=%d offset %d plants %r" % (n, off, plants))


def test_amax_f32_only_raises_slots_and_leaves_the_rest_alone():
    lib = X._lib()
    n = 5000                                                     # five workgroups: slots 0 .. 4 are touched, no other
    t = torch.zeros(n, device="cuda")
    t[4999] = -V
    pre = torch.zeros(AC.SLOTS)
    pre[0] = 2 * V; pre[4] = V / 2; pre[5] = 7.0; pre[1023] = 3.0; pre[600] = 2.0 ** -140
    word = pre.cuda()
    assert lib.sstem_amax_f32(t.data_ptr(), n, word.data_ptr(), None) == 0
    torch.cuda.synchronize()
    got = word.cpu()
    assert bool((got >= pre).all()), "a slot went down"
    want = pre.clone(); want[4] = V                              # element 4999 belongs to workgroup 4 (1024 floats each)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), torch.nonzero(got != want).reshape(-1).tolist()
    # n == 0 leaves the word alone (and reads nothing: the pointer is not looked at)
    before = word.clone()
    assert lib.sstem_amax_f32(None, 0, word.data_ptr(), None) == 0
    assert lib.sstem_amax_f32(t.data_ptr(), 0, word.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(word.view(torch.int32), before.view(torch.int32))
    assert lib.sstem_amax_f32(t.data_ptr(), -1, word.data_ptr(), None) != 0


# ---- the split launches: a maximum made by the convolution or by the epilogue ---------------------------------------------------------------
def _launch_scaled(lib, algo, shape, x, w, flags=0, bias=None, scale=None, shift=None, act=0, slope=0.0, residual=None, res_scale=1.0,
                   layout=X.LAYOUT_NCHW, out=None, x_word=None):
    """sstem_conv3x3_forward_scaled_f32 (the entry without stride and pooled copy); returns (out, word, status)."""
    N, Cin, H, W, Cout = shape
    aid = X.ALGO[algo]
    ws_n = lib.sstem_conv3x3_forward_workspace_floats_algo(N, Cin, H, W, Cout, aid)
    ws = torch.empty(ws_n, device="cuda")
    if out is None:
        out = torch.full((N, Cout, H, W), X.NAN, device="cuda")
    ow = torch.zeros(AC.SLOTS, device="cuda")
    xw = (x_word if x_word is not None else X._word(lib, x)) if algo == "f16x3" else None
    rc = lib.sstem_conv3x3_forward_scaled_f32(_p(x), _p(xw), _p(w), _p(bias), _p(scale), _p(shift), _p(residual), res_scale, _p(out), _p(ow),
                                              _p(ws), ws_n, N, Cin, H, W, Cout, flags, act, slope, None, aid, layout)
    torch.cuda.synchronize()
    return out, ow, rc


class _Plant(object):
    """Operands of the planted launches of one shape: an input that is zero but for ONE element and weights that are zero but for ONE
    centre tap of 1, from the planted input channel into the chosen output channel -- exactly one output element is not zero."""

    def __init__(self, shape, flags=0):
        N, Cin, H, W, Cout = shape
        self.shape, self.flags = shape, flags
        self.x = torch.zeros(N, Cin, H, W, device="cuda")
        self.w = torch.zeros((Cin, Cout, 3, 3) if flags & 1 else (Cout, Cin, 3, 3), device="cuda")

    def ci_of(self, co):
        Cin = self.shape[1]
        return Cin - 1 - co % Cin                                # (channel 0 reads the LAST input channel: the ragged / tap-row chunk)

    def expected(self, pos, v):
        N, Cin, H, W, Cout = self.shape
        ref = torch.zeros(N, Cout, H, W, device="cuda")
        ref[pos] = v
        return ref

    def __call__(self, pos, v):
        """Plant v so that output element pos = (n, co, y, x), and no other, receives it; returns the input."""
        n, co, y, x = pos
        ci = self.ci_of(co)
        self.x.zero_(); self.w.zero_()
        self.x[n, ci, y, x] = v
        if self.flags & 1:
            self.w[ci, co, 1, 1] = 1.0                           # (transposed + flipped: the centre tap stays the centre tap)
        else:
            self.w[co, ci, 1, 1] = 1.0
        return self.x


def _act_of(v, act, slope):
    return v if (act == 0 or v > 0) else (0.0 if act == 1 else v * slope)


def _check_launch(out, ow, rc, ref, want, what):
    sstem_native.check(rc, what)
    if out is not None:
        assert torch.equal(out, ref), "%s: the output is not the planted one (%d elements differ)" % (what, int((out != ref).sum()))
    AC.assert_word(ow, want, what)


@pytest.mark.parametrize("algo", X.IDS)
@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_planted_maximum_forward_scaled(row, algo):
    """sstem_conv3x3_forward_scaled_f32 under X6, X3 and F16X3, unsplit and split over K (the slice-sum launch writes the word)."""
    name, shape, (CO, T, Vv, tail, ks) = row
    N, Cin, H, W, Cout = shape
    lib = X._lib()
    X._supported(lib, shape, algo)
    want_inst = X.Inst(CO, 3 if algo == "x6" else 2, Vv, False, T, tail and algo != "x3", algo == "f16x3", False, False)
    assert X.fwd_instance(algo, shape) == (want_inst, ks, 1) and X._lib_ksplit(lib, shape, algo) == ks
    tw, th = AC.tile_of(T)
    positions = AC.plant_positions(N, Cout, H, W, tw, th, CO)
    assert any(p[1] == Cout - 1 for _, p in positions) and any(p[3] == W - 1 and p[2] == H - 1 and p[0] == N - 1 for _, p in positions)
    plant = _Plant(shape)
    zero = torch.zeros(N, Cout, H, W, device="cuda")
    res = torch.zeros(N, Cout, H, W, device="cuda")
    for pname, pos in positions:
        for sign in SIGNS:
            v = sign * V
            tag = "%s %s %s at %s, V = %r" % (name, algo, pname, pos, v)
            out, ow, rc = _launch_scaled(lib, algo, shape, plant(pos, v), plant.w)
            _check_launch(out, ow, rc, plant.expected(pos, v), V, tag + " (convolution)")
        # the residual makes the maximum: the convolution's output is zero, stored (0 + V) * 0.5
        plant.x.zero_()
        res.zero_(); res[pos] = -V
        ref = torch.zeros_like(res); ref[pos] = -V / 2
        out, ow, rc = _launch_scaled(lib, algo, shape, plant.x, plant.w, residual=res, res_scale=0.5)
        _check_launch(out, ow, rc, ref, V / 2, "%s %s %s at %s (residual, scale 0.5)" % (name, algo, pname, pos))
    # activation on a convolution-made maximum, at the last element
    last = (N - 1, Cout - 1, H - 1, W - 1)
    for act, slope in X.ACTS[1:]:
        stored = _act_of(-V, act, slope)
        out, ow, rc = _launch_scaled(lib, algo, shape, plant(last, -V), plant.w, act=act, slope=slope)
        _check_launch(out, ow, rc, plant.expected(last, stored), abs(stored), "%s %s ReLU / LeakyReLU on a negative maximum, act %d" % (name, algo, act))
    # the epilogue makes the maximum: the bias or the shift of the LAST channel (every pixel of that channel)
    plant.x.zero_()
    ones = torch.ones(Cout, device="cuda")
    for what in ("bias", "shift"):
        for act, slope in X.ACTS:
            for sign in SIGNS:
                v = sign * V
                vec = torch.zeros(Cout, device="cuda"); vec[Cout - 1] = v
                stored = _act_of(v, act, slope)
                ref = zero.clone(); ref[:, Cout - 1] = stored
                kw = {"bias": vec} if what == "bias" else {"scale": ones, "shift": vec}
                out, ow, rc = _launch_scaled(lib, algo, shape, plant.x, plant.w, act=act, slope=slope, **kw)
                _check_launch(out, ow, rc, ref, abs(stored), "%s %s %s of the last channel = %r, act %d" % (name, algo, what, v, act))


def test_planted_maximum_row_segments():
    """SSTEM_LAYOUT_ROW_SEGMENTS with W % 64 != 0: the maximum inside the partial last segment (and everywhere else)."""
    name, shape = X.STORE_ROW
    N, Cin, H, W, Cout = shape
    lib = X._lib()
    X._supported(lib, shape, "f16x3")
    assert W % 64 != 0 and X.fwd_instance("f16x3", shape, layout=X.LAYOUT_ROWSEG)[0] == X.Inst(32, 2, True, False, 32, False, True, False, False)
    TX = X._cdiv(W, 64)
    plant = _Plant(shape)
    positions = AC.plant_positions(N, Cout, H, W, 32, 8, 32) + [("partial_first", (0, 3, 5, W - W % 64)), ("partial_inner", (0, Cout - 1, H - 1, W - W % 64 + 7))]
    for pname, pos in positions:
        for sign in SIGNS:
            seg = torch.full((N, H, TX, Cout, 64), X.NAN, device="cuda")
            _, ow, rc = _launch_scaled(lib, "f16x3", shape, plant(pos, sign * V), plant.w, layout=X.LAYOUT_ROWSEG, out=seg)
            flat = seg.permute(0, 3, 1, 2, 4).reshape(N, Cout, H, TX * 64)
            _check_launch(flat[..., :W], ow, rc, plant.expected(pos, sign * V), V, "row segments %s at %s" % (pname, pos))
            assert bool(torch.isnan(flat[..., W:]).all())


def test_planted_maximum_channel_block_and_pooled_copies():
    """sstem_conv3x3_forward_scaled_strided_f32: the store into a channel block of a larger tensor; the pooled copy (max, average) with
    the full-resolution output and with output == NULL.  The word bounds the FULL-RESOLUTION values the launch computes (|V|), which
    bound the pooled ones (hipnn hands the same word to both tensors)."""
    name, shape = X.STORE_ROW
    N, Cin, H, W, Cout = shape
    lib = X._lib()
    plant = _Plant(shape)
    for pname, pos in AC.plant_positions(N, Cout, H, W, 32, 8, 32):
        for sign in SIGNS:
            v = sign * V
            ref = plant.expected(pos, v)
            x = plant(pos, v)
            big = torch.full((N, Cout + 5, H, W), X.NAN, device="cuda")
            _, _, ow, rc = X._launch_fwd(lib, "f16x3", shape, x, plant.w, 0, out=big, out_ptr=big[0, 5].data_ptr(), out_stride=(Cout + 5) * H * W)
            _check_launch(big[:, 5:], ow, rc, ref, V, "channel block %s at %s" % (pname, pos))
            assert bool(torch.isnan(big[:, :5]).all())
            for kind in (1, 2):
                pref = CE.pool2x2_ref64(ref.double(), kind).float()
                for want_out in (True, False):
                    pooled = torch.full((N, Cout, H // 2, W // 2), X.NAN, device="cuda")
                    out, _, ow, rc = X._launch_fwd(lib, "f16x3", shape, x, plant.w, 0, pooled=pooled, pool_kind=kind, want_out=want_out)
                    tag = "pooled copy kind %d, full-resolution output %s, %s at %s, V = %r" % (kind, want_out, pname, pos, v)
                    _check_launch(out, ow, rc, ref, V, tag)
                    assert torch.equal(pooled, pref), tag
                    assert float(pooled.abs().max()) <= float(ow.max())


def test_planted_maximum_sub_pixel_conv_transpose():
    """SSTEM_LAYOUT_CONVT_PARITY: one plant per output parity (channel par * C + co of the launch is pixel parity par of channel co)."""
    N, Cin, H, W, C = X.CT_TILE_SHAPE
    shape = (N, Cin, H, W, 4 * C)
    lib = X._lib()
    X._supported(lib, shape, "f16x3")
    assert X.fwd_instance("f16x3", shape, layout=X.LAYOUT_CT)[0] == X.Inst(64, 2, True, False, 32, False, True, False, True)
    plant = _Plant(shape)                                         # tap (1, 1) of the 2 x 2 window: output (2y + py, 2x + px) reads in[y][x]
    for pname, (n, co, y, x) in AC.plant_positions(N, C, H, W, 32, 8, 32):
        for par in range(4):
            v = V if par % 2 else -V
            out = torch.full((N, C, 2 * H, 2 * W), X.NAN, device="cuda")
            xin = plant((n, par * C + co, y, x), v)
            _, _, ow, rc = X._launch_fwd(lib, "f16x3", shape, xin, plant.w, 0, layout=X.LAYOUT_CT, out=out)
            ref = torch.zeros_like(out)
            ref[n, co, 2 * y + (par >> 1), 2 * x + (par & 1)] = v
            _check_launch(out, ow, rc, ref, V, "sub-pixel ConvTranspose %s at %s parity %d" % (pname, (n, co, y, x), par))


@pytest.mark.parametrize("cout", [1, 2, 3, 4, 6, 8])
def test_planted_maximum_streaming_small_cout(cout):
    """SSTEM_CONV_DIRECT of the strided entry (the streaming kernel: 256 x 8 tiles, one plane per output channel)."""
    shape = (2, 5, 20, 36, cout)
    N, Cin, H, W, Cout = shape
    lib = X._lib()
    assert lib.sstem_conv3x3_stream_small_supported(N, Cin, H, W, Cout) == 1
    plant = _Plant(shape)
    for pname, pos in AC.plant_positions(N, Cout, H, W, 256, 8, 8):
        for sign in SIGNS:
            v = sign * V
            out = torch.full((N, Cout, H, W), X.NAN, device="cuda"); ow = torch.zeros(AC.SLOTS, device="cuda")
            rc = lib.sstem_conv3x3_forward_scaled_strided_f32(_p(plant(pos, v)), None, _p(plant.w), None, None, None, None, 1.0, _p(out), _p(ow),
                                                              None, 0, N, Cin, H, W, Cout, 0, 0, 0.0, None, HF.ALGO_DIRECT, 0, 0, None, 0)
            torch.cuda.synchronize()
            _check_launch(out, ow, rc, plant.expected(pos, v), V, "streaming kernel Cout=%d %s at %s" % (cout, pname, pos))
    bias = torch.zeros(Cout, device="cuda"); bias[Cout - 1] = -V
    plant.x.zero_()
    for act, slope in X.ACTS:
        out = torch.full((N, Cout, H, W), X.NAN, device="cuda"); ow = torch.zeros(AC.SLOTS, device="cuda")
        rc = lib.sstem_conv3x3_forward_scaled_strided_f32(_p(plant.x), None, _p(plant.w), _p(bias), None, None, None, 1.0, _p(out), _p(ow),
                                                          None, 0, N, Cin, H, W, Cout, 0, act, slope, None, HF.ALGO_DIRECT, 0, 0, None, 0)
        torch.cuda.synchronize()
        stored = _act_of(-V, act, slope)
        ref = torch.zeros_like(out); ref[:, Cout - 1] = stored
        _check_launch(out, ow, rc, ref, abs(stored), "streaming kernel Cout=%d bias of the last channel, act %d" % (cout, act))


MASK_ROWS = [r for r in ROWS if r[2][2]]                          # (the masked fp16 instances exist behind the 16-byte staging only)


@pytest.mark.parametrize("flags", [0, 1], ids=["forward", "transposed"])
@pytest.mark.parametrize("row", MASK_ROWS, ids=[r[0] for r in MASK_ROWS])
def test_planted_maximum_masked_launches(row, flags):
    """sstem_conv3x3_forward_scaled_masked_f32, forward and transposed: an input_mask that zeroes the planted element leaves the word
    all-zero; one that zeroes another element leaves |V|."""
    name, shape, (CO, T, Vv, tail, ks) = row
    N, Cin, H, W, Cout = shape
    lib = X._lib()
    X._supported(lib, shape, "f16x3")
    assert X.fwd_instance("f16x3", shape, masked=True)[0] == X.Inst(CO, 2, Vv, True, T, tail, True, False, False)
    tw, th = AC.tile_of(T)
    plant = _Plant(shape, flags)
    for pname, pos in AC.plant_positions(N, Cout, H, W, tw, th, CO):
        n, co, y, x = pos
        for hide in (False, True):
            v = -V if hide else V
            xin = plant(pos, v)
            xw = X._word(lib, xin)
            mask = torch.ones(N, Cin, H, W, dtype=torch.bool, device="cuda")
            mask[n, plant.ci_of(co), y, x] = not hide
            mask[n, plant.ci_of(co), (y + 1) % H, x] = False       # (an element that holds zero anyway)
            out, om, ow, rc = X._launch_fwd(lib, "f16x3", shape, xin, plant.w, flags, in_mask=mask, want_mask=True, x_word=xw)
            ref = plant.expected(pos, 0.0 if hide else v)
            tag = "%s flags=%d %s at %s, planted element %s" % (name, flags, pname, pos, "masked out" if hide else "kept")
            _check_launch(out, ow, rc, ref, 0.0 if hide else V, tag)
            assert torch.equal(om, ref > 0), tag + ": output mask"


def test_planted_maximum_first_layer_u8():
    """sstem_conv3x3_first_layer_u8: one byte 255 (= 1.0) in either frame, a centre-tap weight of V into one output channel."""
    N, H, W, Cout = 2, 20, 36, 6
    lib = X._lib()
    assert lib.sstem_conv3x3_first_layer_u8_supported(N, H, W, Cout) == 1
    frames = torch.zeros(N, 2, H, W, dtype=torch.uint8, device="cuda")
    for k, (pname, (n, co, y, x)) in enumerate(AC.plant_positions(N, Cout, H, W, 256, 8, 8)):
        for frame in (0, 1):
            for act in (0, 1):
                v = -V if (act or (k + frame) % 2) else V
                frames.zero_(); frames[n, frame, y, x] = 255
                w = torch.zeros(6, 6, 3, 3, device="cuda"); w[co, 3 * frame + k % 3, 1, 1] = v
                out = torch.full((N, 6, H, W), X.NAN, device="cuda"); planes = torch.full((2, N, H, W), X.NAN, device="cuda")
                ow = torch.zeros(AC.SLOTS, device="cuda")
                rc = lib.sstem_conv3x3_first_layer_u8(_p(frames), _p(w), None, _p(out), _p(planes), _p(ow), N, H, W, Cout, act, 0.0, None)
                torch.cuda.synchronize()
                stored = _act_of(v, act, 0.0)
                ref = torch.zeros_like(out); ref[n, co, y, x] = stored
                _check_launch(out, ow, rc, ref, abs(stored), "u8 first layer %s at %s frame %d act %d" % (pname, (n, co, y, x), frame, act))
                assert float(planes.sum()) == 1.0 and float(planes[frame, n, y, x]) == 1.0


# ---- fp16 weight packing: the per-layer form and the group form ---------------------------------------------------------------------------
PACK_LAYERS = [(20, 24), (32, 40), (17, 33)]                     # (Cin, Cout); 4320 / 11520 / 5049 weights: ragged blocks of the bound launch


def _pack_group(lib, ws):
    """sstem_conv3x3_pack_weights_group_f16 over `ws` (include/sstem_conv.h: the table); returns (forward images, transposed images, bounds)."""
    rows, first, first_b = [], 0, 0
    bounds = torch.full((len(ws),), 9.0e9, device="cuda")         # (cleared by the entry point)
    outs_f, outs_t = [], []
    for i, w in enumerate(ws):
        Cout, Cin = w.shape[:2]
        entry = (ctypes.c_int64 * 16)()
        blocks = int(lib.sstem_conv3x3_pack_group_entry(Cin, Cout, F16, entry))
        e = list(entry)
        f = torch.full((lib.sstem_conv3x3_packed_floats(Cin, Cout, F16),), X.NAN, device="cuda")
        t = torch.full((lib.sstem_conv3x3_packed_floats(Cout, Cin, F16),), X.NAN, device="cuda")
        outs_f.append(f); outs_t.append(t)
        nb = e[14]
        e[0], e[1], e[2], e[13], e[14], e[15] = w.data_ptr(), f.data_ptr(), t.data_ptr(), first, first_b, bounds.data_ptr() + 4 * i
        first += blocks; first_b += nb
        rows.append(e)
    table = torch.tensor(rows, dtype=torch.int64, device="cuda")
    rc = lib.sstem_conv3x3_pack_weights_group_f16(table.data_ptr(), len(ws), first, first_b, bounds.data_ptr(), None)
    torch.cuda.synchronize()
    sstem_native.check(rc, "sstem_conv3x3_pack_weights_group_f16")
    return outs_f, outs_t, bounds


@pytest.mark.parametrize("entry,last", [(0, False), (0, True), (2, False), (2, True)], ids=["first_first", "first_last", "last_first", "last_last"])
def test_fp16_packing_bounds_the_first_and_the_last_weight(entry, last):
    """The largest weight at the first / last element of the first / last entry of a three-layer table, 2^3 times the rest (a missed
    element moves the scale by three binades): the per-layer form measures it, and the group form gives the per-layer form's bounds
    and image bytes bit for bit."""
    lib = X._lib()
    g = torch.Generator().manual_seed(7 + 2 * entry + last)
    ws = [(torch.rand(co, ci, 3, 3, generator=g) * 2 - 1).cuda() for ci, co in PACK_LAYERS]
    big = -8.0 if last else 8.0
    ws[entry].view(-1)[-1 if last else 0] = big
    gf, gt, bounds = _pack_group(lib, ws)
    for i, w in enumerate(ws):
        Cout, Cin = w.shape[:2]
        n_f = lib.sstem_conv3x3_packed_floats(Cin, Cout, F16) - AC.SLOTS       # (the word behind the image is scratch of the per-layer form)
        n_t = lib.sstem_conv3x3_packed_floats(Cout, Cin, F16) - AC.SLOTS
        rf = torch.full((n_f + AC.SLOTS,), X.NAN, device="cuda"); rt = torch.full((n_t + AC.SLOTS,), X.NAN, device="cuda")
        assert lib.sstem_conv3x3_pack_weights_f32(w.data_ptr(), Cin, Cout, F16, rf.data_ptr(), rt.data_ptr(), None) == 0
        torch.cuda.synchronize()
        true = float(w.abs().max())
        assert true == (8.0 if i == entry else true) and (i == entry or true < 1.0)
        assert float(rf[0]) == true == float(rt[0]), "layer %d: the per-layer form's bound %r, largest weight %r" % (i, float(rf[0]), true)
        word = rf[n_f:]                                           # (one slot per workgroup of sstem_amax_f32's pass, each its own maximum)
        assert float(word.max()) == true and float(word.min()) >= 0.0, "layer %d: the word the per-layer form measured" % i
        assert float(bounds[i]) == true == float(gf[i][0]) == float(gt[i][0]), "layer %d: the group form's bound" % i
        assert torch.equal(gf[i][4:n_f].view(torch.int32), rf[4:n_f].view(torch.int32)), "layer %d: forward image" % i
        assert torch.equal(gt[i][4:n_t].view(torch.int32), rt[4:n_t].view(torch.int32)), "layer %d: transposed image" % i


# ---- consumers: where the bound lives and how large it is ------------------------------------------------------------------------------------
FWD_SWEEP_SHAPE = X.FWD_ROWS[0][1]                                # co32_vec (1, 32, 9, 36, 20)
WGRAD_SWEEP_SHAPE = X.WGRAD_ROWS[0][1]                            # vec (2, 40, 9, 36, 70): ten slabs


def _with_max(t, bound):
    """t scaled so that its largest magnitude is exactly `bound` (one element set to it, the rest below)."""
    t = t * (0.75 * bound / float(t.abs().max()))
    t.view(-1)[t.numel() // 3] = -bound
    assert float(t.abs().max()) == bound
    return t


def _fwd_under(lib, x, w, b, word):
    out, _, _, rc = X._launch_fwd(lib, "f16x3", FWD_SWEEP_SHAPE, x, w, 0, b, x_word=word)
    sstem_native.check(rc, "split convolution launch")
    return out


def _wgrad_under(lib, x, g, xw, gw_):
    N, Cin, H, W, Cout = WGRAD_SWEEP_SHAPE
    ws_n = lib.sstem_conv3x3_wgrad_workspace_floats_algo(N, Cin, H, W, Cout, F16)
    ws = torch.empty(ws_n, device="cuda")
    gw = torch.full((Cout, Cin, 3, 3), X.NAN, device="cuda"); gb = torch.full((Cout,), X.NAN, device="cuda")
    rc = lib.sstem_conv3x3_backward_weight_scaled_masked_f32(_p(x), _p(xw), _p(g), _p(gw_), None, _p(gw), _p(gb), _p(ws), ws_n, N, Cin, H, W,
                                                             Cout, 0, None)
    torch.cuda.synchronize()
    sstem_native.check(rc, "split weight gradient launch")
    return gw, gb


def test_slot_sweep_the_bound_may_live_in_any_slot():
    """amax_word_max (64 lanes x four 16-byte loads): the same bound in slot 0, 3, 4, 255, 256, 511, 1023 alone, or in every slot, gives
    bit-identical outputs -- forward and weight gradient (either word)."""
    lib = X._lib()
    g = torch.Generator().manual_seed(31)
    N, Cin, H, W, Cout = FWD_SWEEP_SHAPE
    x = _with_max(torch.randn(N, Cin, H, W, generator=g), 3.0).cuda()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * 0.2).cuda(); b = torch.randn(Cout, generator=g).cuda()
    base = _fwd_under(lib, x, w, b, X._word(lib, x))
    _close(base, CE.conv_ref64(x, w, b))
    for slot in AC.SWEEP_SLOTS + ("all",):
        got = _fwd_under(lib, x, w, b, AC.hand_word(3.0, slot, "cuda"))
        assert torch.equal(got.view(torch.int32), base.view(torch.int32)), "forward: bound in slot %s" % (slot,)
    N, Cin, H, W, Cout = WGRAD_SWEEP_SHAPE
    x = _with_max(torch.randn(N, Cin, H, W, generator=g), 3.0).cuda()
    gr = _with_max(torch.randn(N, Cout, H, W, generator=g), 2.0 ** -9).cuda()
    bw, bb = _wgrad_under(lib, x, gr, X._word(lib, x), X._word(lib, gr))
    rw, rb = CE.conv_wgrad_ref64(x, gr)
    _close(bw, rw); _close(bb, rb)
    for slot in AC.SWEEP_SLOTS + ("all",):
        for which in (0, 1):
            xw = AC.hand_word(3.0, slot if which == 0 else 0, "cuda")
            gw_ = AC.hand_word(2.0 ** -9, slot if which == 1 else 1023, "cuda")
            gw, gb = _wgrad_under(lib, x, gr, xw, gw_)
            assert torch.equal(gw.view(torch.int32), bw.view(torch.int32)) and torch.equal(gb.view(torch.int32), bb.view(torch.int32)), \
                "weight gradient: bound of %s in slot %s" % (("input", "gradient")[which], slot)


# (what the tensor's largest magnitude is, what the word says).  "2^k exactly" and its predecessor sit on either side of a binade's
# edge; 2^-111 and below reach the clamp e < 16 (csrc/conv_split_common.h amax_exponent); 2^124 and above reached a clamp e > 250 that
# sent maxima of 2^125 and more to fp16 inf -- these cases found it, and the clamp is gone (every finite bound has a normal scale); a word
# above the true maximum costs precision only beyond 18 binades (include/sstem_conv.h).
P2 = [2.0 ** k for k in (-20, 0, 1, 13, 40)]
BOUND_CASES = [(v, v) for v in P2] + [(AC.predecessor(v), AC.predecessor(v)) for v in P2] + \
              [(2.0 ** -111, 2.0 ** -111), (2.0 ** -120, 2.0 ** -120), (2.0 ** -130, 2.0 ** -130), (2.0 ** -140, 2.0 ** -140)] + \
              [(2.0 ** 123, 2.0 ** 123), (2.0 ** 124, 2.0 ** 124), (2.0 ** 126, 2.0 ** 126), (AC.predecessor(2.0 ** 127) * 2, AC.predecessor(2.0 ** 127) * 2)] + \
              [(3.0, float("inf")), (1000.0, float("inf"))] + \
              [(3.0, 3.0 * 2.0 ** k) for k in (1, 2, 3)] + [(2.0 ** 13, 2.0 ** 16), (AC.predecessor(2.0), 16.0)]


def _held(got, ref, S, what):
    """Finite wherever the float64 result is representable, and within the id's tolerance (``_close``) of it.  An element counts where
    the sum of its terms' MAGNITUDES, S, stays below 2^127: there no partial sum of an fp32 evaluation, in any order, overflows."""
    ok = S < 2.0 ** 127
    assert bool(ok.any()), what + ": no element of this case is representable"
    bad = ok & ~torch.isfinite(got)
    assert not bool(bad.any()), "%s: %d non-finite values where the float64 result is finite" % (what, int(bad.sum()))
    zero = torch.zeros((), dtype=torch.float64, device=ref.device)
    _close(torch.where(ok, got.double(), zero), torch.where(ok, ref, zero))


def _other_scale(bound):
    """A power of two for the OTHER operand that brings the products near 1 (kept inside float32's normal range)."""
    import math
    return 2.0 ** max(-100, min(100, -int(math.floor(math.log2(bound)))))


@pytest.mark.parametrize("true_max,bound", BOUND_CASES, ids=["max%.9g_word%.9g" % c for c in BOUND_CASES])
def test_binade_and_clamp_sweep_forward(true_max, bound):
    lib = X._lib()
    g = torch.Generator().manual_seed(41)
    N, Cin, H, W, Cout = FWD_SWEEP_SHAPE
    x = _with_max(torch.randn(N, Cin, H, W, generator=g), true_max).cuda()
    ws = _other_scale(true_max)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * 0.2 * ws).cuda(); b = (torch.randn(Cout, generator=g)).cuda()
    ref, S = CE.conv_ref64(x, w, b), CE.conv_ref64(x.abs(), w.abs(), b.abs())
    assert bool((S < 2.0 ** 127).all())                          # (every output of the forward cases is representable)
    out = _fwd_under(lib, x, w, b, AC.hand_word(bound, 517, "cuda"))
    print("largest |x| %.6g under a bound of %.6g (scale 2^%d): max error %.3e of max|ref| %.3e" % (
        true_max, bound, AC.scale_log2(bound), float((out.double() - ref).abs().max()), float(ref.abs().max())))
    _held(out, ref, S, "forward")


@pytest.mark.parametrize("true_max,bound", BOUND_CASES, ids=["max%.9g_word%.9g" % c for c in BOUND_CASES])
def test_binade_and_clamp_sweep_weight_gradient(true_max, bound):
    """Both words: the case's (maximum, bound) on the input with a gradient that brings the sums near 1, then the other way round."""
    lib = X._lib()
    g = torch.Generator().manual_seed(43)
    N, Cin, H, W, Cout = WGRAD_SWEEP_SHAPE
    other = _other_scale(true_max) * 2.0 ** -6
    for which in (0, 1):
        a = _with_max(torch.randn(N, Cin if which == 0 else Cout, H, W, generator=g), true_max).cuda()
        o = _with_max(torch.randn(N, Cout if which == 0 else Cin, H, W, generator=g), other).cuda()
        x, gr = (a, o) if which == 0 else (o, a)
        wa, wo = AC.hand_word(bound, 1022, "cuda"), AC.hand_word(other, 1, "cuda")
        xw, gw_ = (wa, wo) if which == 0 else (wo, wa)
        rw, rb = CE.conv_wgrad_ref64(x, gr)
        Sw, Sb = CE.conv_wgrad_ref64(x.abs(), gr.abs())
        assert bool((Sw < 2.0 ** 127).all())                      # (the bias gradient of a huge gradient tensor may not be: a plain fp32 sum)
        gw, gb = _wgrad_under(lib, x, gr, xw, gw_)
        tag = "bound on the %s" % ("input", "gradient")[which]
        _held(gw, rw, Sw, "weight gradient, " + tag)
        if bool((Sb < 2.0 ** 127).any()):
            _held(gb, rb, Sb, "bias gradient, " + tag)


def test_all_zero_tensor_under_a_zero_word():
    lib = X._lib()
    g = torch.Generator().manual_seed(47)
    N, Cin, H, W, Cout = FWD_SWEEP_SHAPE
    x = torch.zeros(N, Cin, H, W, device="cuda")
    w = torch.randn(Cout, Cin, 3, 3, generator=g).cuda(); b = torch.randn(Cout, generator=g).cuda()
    out = _fwd_under(lib, x, w, b, torch.zeros(AC.SLOTS, device="cuda"))
    assert torch.equal(out, b.view(1, -1, 1, 1).expand_as(out))
    N, Cin, H, W, Cout = WGRAD_SWEEP_SHAPE
    x = torch.zeros(N, Cin, H, W, device="cuda"); gr = torch.randn(N, Cout, H, W, generator=g).cuda()
    gw, gb = _wgrad_under(lib, x, gr, torch.zeros(AC.SLOTS, device="cuda"), X._word(lib, gr))
    assert not bool(gw.any())
    _close(gb, gr.double().sum((0, 2, 3)))
    gw, gb = _wgrad_under(lib, gr[:, :Cin].contiguous(), torch.zeros(N, Cout, H, W, device="cuda"), X._word(lib, gr), torch.zeros(AC.SLOTS, device="cuda"))
    assert not bool(gw.any()) and not bool(gb.any())
