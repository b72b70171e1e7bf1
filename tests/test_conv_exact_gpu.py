"""The convolution ids bit for bit on exactly summable inputs (tests/conv_exact.py: the domains, the budget rule, the references).

Every assertion on a kernel's output here is ``torch.equal(got.double(), ref)`` at every element -- the inputs are built so that every
product an id promises (include/sstem_conv.h) and every partial sum in any order is an fp32 number, which each case ASSERTS of its own
inputs (``exact_domain``, ``assert_exactly_summable``, the reference equal to its own fp32 rounding) before it looks at the output.  The
one bound that appears is F16X3's one-hot statement, copied from the header: |out - x| <= 2^-22 |x| + 2^-25 bound.

The dispatch rules of the two split launchers (csrc/conv_split_kernels.hip: split_wt16, split_geom, split_tail_chunk, the `vec` and
`walk` rules; csrc/conv_split_wgrad.hip: wgrad_split_plan) are restated below; every row of the tables states the instance it is meant
to reach, each case asserts that the restated rules send it there and -- where the library exposes it (the K slices, through the
workspace queries) -- that the library agrees, and a module-level check asserts that the tables reach every instance the launchers
can dispatch to.  A shape the library refuses fails its case; nothing skips."""
import collections

import pytest
import torch

import conv_exact as CE
import hipnn.functional as HF
import sstem_native
from test_conv_f16train_gpu import _word
from test_conv_gpu import CONVT_SHAPES, SHAPES as FP32_SHAPES, SPLITK_SHAPES, _c_forward

pytestmark = pytest.mark.gpu

ALGO = {"x6": HF.ALGO_MFMA_BF16X6, "x3": HF.ALGO_MFMA_BF16X3, "f16x3": HF.ALGO_MFMA_F16X3}
IDS = ("x6", "x3", "f16x3")
LAYOUT_NCHW, LAYOUT_ROWSEG, LAYOUT_CT = 0, 1, 2
NAN = float("nan")


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in ("SSTEM_SPLIT_WALK", "SSTEM_SPLIT_WALK_MIN_WGS", "SSTEM_SPLIT_WALK_CT", "SSTEM_WGRAD_PINGPONG"):
        monkeypatch.delenv(k, raising=False)
    yield
    HF.set_algorithm(HF.ALGO_AUTO)


# ---- the launchers' dispatch, restated ---------------------------------------------------------------------------------------------------
# (csrc/conv_split_kernels.hip: split_forward_plan decides -- CO, ncb, ksplit, vec, w16, tail, masked, walk, ct, ctwalk, grid, or a
# refusal -- and launch_conv3x3_split_mfma dispatches on that struct; fwd_instance below is that plan for 16-byte aligned tensors)
# conv3x3_split_mfma<A, B, P, V, M, T, TL, F16, DEEP, CT>: CO = 32 (A, B = 1, 4) or 64 (2, 2) output channels per workgroup, P pieces,
# V 16-byte staging, M masked, T tile width (16: 16 x 16 tiles, 32: 32 x 8), TL tap-row last chunk, DEEP tile-walking, CT sub-pixel store
Inst = collections.namedtuple("Inst", "CO P V M T TL F16 DEEP CT")
# conv3x3_wgrad_split_mfma<P, V, M, F16, PP>
WInst = collections.namedtuple("WInst", "P V M F16 PP")


def _cdiv(a, b):
    return (a + b - 1) // b


def split_wt16(W):
    return W <= 16 and W % 4 == 0


def split_tail_chunk(cin, pieces, f16):
    return (pieces == 3 or f16) and cin > 16 and 1 <= cin % 16 <= 4


def split_geom(N, Cin, H, W, Cout):
    """(CO, ncb, ksplit): 64 channels per workgroup above 32 outputs; K slices of whole chunks, at least two chunks each, while the
    grid is below 512 workgroups."""
    w16 = split_wt16(W)
    tw, th = (16, 16) if w16 else (32, 8)
    tiles = _cdiv(W, tw) * _cdiv(H, th) * N
    nchunks = _cdiv(Cin, 16)
    CO = 32 if Cout <= 32 else 64
    ncb = _cdiv(Cout, CO)
    ks = 1
    while tiles * ncb * ks < 512 and ks < 8 and nchunks % (ks * 2) == 0 and nchunks // (ks * 2) >= 2:
        ks *= 2
    return CO, ncb, ks


def fwd_instance(algo, shape, masked=False, layout=LAYOUT_NCHW, strided=False, pooled=False, walk=8, walk_min=2048):
    """(Inst, ksplit, tiles walked) of launch_conv3x3_split_mfma for 16-byte aligned tensors; None where the launcher refuses."""
    N, Cin, H, W, Cout = shape
    f16, P = algo == "f16x3", 3 if algo == "x6" else 2
    CO, ncb, ks = split_geom(N, Cin, H, W, Cout)
    ksplit = 1 if (layout or strided or pooled) else ks
    vec = W % 4 == 0 and (not f16 or H * W * 32 < 2 ** 31)
    w16 = vec and split_wt16(W)
    tw, th = (16, 16) if w16 else (32, 8)
    gx, gy, gz = _cdiv(W, tw), _cdiv(H, th), N * ncb * ksplit
    tail = split_tail_chunk(Cin, P, f16)
    if layout == LAYOUT_CT:
        if not (f16 and Cout % 128 == 0 and Cin % 16 == 0 and vec and not w16 and not tail and CO == 64):
            return None
        cw = 8
        while cw > 1 and gx * _cdiv(gy, cw) * gz < 2048:
            cw >>= 1
        return Inst(64, 2, True, False, 32, False, True, cw >= 2, True), 1, cw
    wk = 0
    if f16 and vec and not w16 and not tail and ksplit == 1 and walk > 0 and CO == 32 and not masked:
        wk = walk
        while wk > 1 and gx * _cdiv(gy, wk) * gz < walk_min:
            wk >>= 1
        if wk < 2:
            wk = 0
    if wk:
        return Inst(32, 2, True, False, 32, False, True, True, False), 1, wk
    if f16 and masked and not vec:
        return None
    return Inst(CO, P, vec, masked, 16 if w16 else 32, tail if (P == 3 or f16) else False, f16, False, False), ksplit, 1


def wgrad_split_plan(N, Cin, H, W, Cout):
    """(CinP, CoutP, ksplit): 2-row x 32-column pixel tiles dealt to 256 / (64 x 64 channel blocks) workgroups, at least two tiles each."""
    CinP, CoutP = _cdiv(Cin, 64) * 64, _cdiv(Cout, 64) * 64
    ntiles = N * _cdiv(W, 32) * _cdiv(H, 2)
    blocks = (CinP // 64) * (CoutP // 64)
    return CinP, CoutP, max(1, min(_cdiv(256, blocks), ntiles // 2))


def wgrad_instance(algo, shape, masked, pingpong=True):
    f16 = algo == "f16x3"
    return WInst(3 if algo == "x6" else 2, shape[3] % 4 == 0, masked, f16, f16 and pingpong)


def _all_fwd_instances():
    s = set()
    for CO in (32, 64):
        for V, T in ((True, 16), (True, 32), (False, 32)):
            for M in (False, True):
                s.update(Inst(CO, 3, V, M, T, TL, False, False, False) for TL in (False, True))
                s.add(Inst(CO, 2, V, M, T, False, False, False, False))
                if V or not M:                                # (the masked fp16 instances exist for the 16-byte staging only)
                    s.update(Inst(CO, 2, V, M, T, TL, True, False, False) for TL in (False, True))
    s.add(Inst(32, 2, True, False, 32, False, True, True, False))
    s.add(Inst(64, 2, True, False, 32, False, True, False, True))
    s.add(Inst(64, 2, True, False, 32, False, True, True, True))
    return s


def _all_wgrad_instances():
    s = {WInst(P, V, M, False, False) for P in (3, 2) for V in (True, False) for M in (True, False)}
    return s | {WInst(2, V, M, True, PP) for V in (True, False) for M in (True, False) for PP in (True, False)}


# ---- the tables ----------------------------------------------------------------------------------------------------------------------------
# (name, (N, Cin, H, W, Cout), the instance the row is there for: CO, T, V, tap-row last chunk (X6 and F16X3), K slices)
FWD_ROWS = [
    ("co32_vec", (1, 32, 9, 36, 20), (32, 32, True, False, 1)),
    ("co64_vec", (2, 32, 9, 36, 70), (64, 32, True, False, 1)),
    ("co32_dword", (1, 32, 9, 37, 20), (32, 32, False, False, 1)),
    ("co64_dword", (1, 32, 9, 37, 70), (64, 32, False, False, 1)),
    ("co64_t16", (2, 48, 17, 16, 40), (64, 16, True, False, 1)),
    ("co32_t16_ragged", (1, 32, 24, 12, 32), (32, 16, True, False, 1)),
    ("tail1", (1, 17, 9, 36, 20), (32, 32, True, True, 1)),
    ("tail4", (1, 20, 9, 36, 20), (32, 32, True, True, 1)),
    ("tail3_of_51", (1, 51, 9, 36, 20), (32, 32, True, True, 2)),          # (four chunks: two K slices, the tap-row chunk in the second)
    ("pad22", (1, 22, 9, 36, 20), (32, 32, True, False, 1)),
    ("pad6", (1, 6, 9, 36, 20), (32, 32, True, False, 1)),
    ("ksplit4", (2, 128, 16, 16, 64), (64, 16, True, False, 4)),
    # the tap-row chunk under the other staging / tile / channel-block forms (the dispatch has an instance for each)
    ("tail_co64_vec", (1, 20, 9, 36, 70), (64, 32, True, True, 1)),
    ("tail_co32_dword", (1, 19, 9, 37, 20), (32, 32, False, True, 1)),
    ("tail_co64_dword", (1, 18, 9, 37, 70), (64, 32, False, True, 1)),
    ("tail_co64_t16", (1, 20, 17, 16, 40), (64, 16, True, True, 1)),
    ("tail_co32_t16", (1, 17, 24, 12, 32), (32, 16, True, True, 1)),
]
ONE_HOT_ROWS = FWD_ROWS[:12]
WALK_ROW = ("walk8_ragged", (1, 32, 72, 64, 32))                 # SSTEM_SPLIT_WALK=8, _MIN_WGS=1: nine tile rows = groups of 8 + 1
STORE_ROW = ("stores", (1, 32, 16, 96, 32))                      # row segments, channel block of a larger tensor, pooled copies
CT_TILE_SHAPE = (1, 16, 9, 20, 32)                               # (N, Cin, H, W, C): the per-tile sub-pixel instance
MASKS = ("in", "out", "both")

WGRAD_ROWS = [
    ("vec", (2, 40, 9, 36, 70), 10),
    ("dword", (1, 24, 9, 37, 33), 5),
    ("odd_rows", (3, 64, 5, 64, 64), 9),
    ("one_slice", (1, 20, 3, 20, 24), 1),
]


def _ct_walk_shape():
    """The smallest H at (1, 16, H, 128, 32) that the launcher walks: 2048 workgroups left at two tiles per workgroup."""
    H = 8
    while not fwd_instance("f16x3", (1, 16, H, 128, 128), layout=LAYOUT_CT)[0].DEEP:
        H += 8
    return (1, 16, H - 7, 128, 32)                                # (the last tile row one pixel high: same grid)


CT_WALK_SHAPE = _ct_walk_shape()


def _reached():
    fwd, ksplits, wg = set(), set(), set()
    for _, shape, _ in FWD_ROWS:
        for algo in IDS:
            for masked in (False, True):
                r = fwd_instance(algo, shape, masked)
                if r is not None:
                    fwd.add(r[0]); ksplits.add(r[1])
    fwd.add(fwd_instance("f16x3", WALK_ROW[1], walk=8, walk_min=1)[0])
    for shape in (CT_TILE_SHAPE, CT_WALK_SHAPE):
        fwd.add(fwd_instance("f16x3", shape[:4] + (4 * shape[4],), layout=LAYOUT_CT)[0])
    for _, shape, _ in WGRAD_ROWS:
        for algo in IDS:
            for masked in (False, True):
                for pp in ((True, False) if algo == "f16x3" else (True,)):
                    wg.add(wgrad_instance(algo, shape, masked, pp))
    return fwd, ksplits, wg


_FWD_REACHED, _KSPLITS_REACHED, _WGRAD_REACHED = _reached()
assert _FWD_REACHED == _all_fwd_instances(), sorted(_all_fwd_instances() - _FWD_REACHED)
assert _WGRAD_REACHED == _all_wgrad_instances(), sorted(_all_wgrad_instances() - _WGRAD_REACHED)
assert {1, 4} <= _KSPLITS_REACHED                                 # the launch's own store and the slice-sum launch
assert fwd_instance("f16x3", CT_WALK_SHAPE[:4] + (128,), layout=LAYOUT_CT)[2] == 2 and CT_WALK_SHAPE == (1, 16, 4081, 128, 32)
assert {p[2] for p in WGRAD_ROWS} >= {1} and max(p[2] for p in WGRAD_ROWS) >= 4


# ---- helpers -------------------------------------------------------------------------------------------------------------------------------
def _lib():
    return sstem_native.load_library()


def _p(t):
    return None if t is None else t.data_ptr()


def _cuda(*ts):
    return [None if t is None else t.cuda() for t in ts]


def _eq(got, ref, what):
    g = got.double()
    if not torch.equal(g, ref):
        bad = torch.nonzero(g != ref)
        raise AssertionError("%s: %d of %d elements differ from the float64 reference; first at %s: got %r, want %r"
                             % (what, bad.shape[0], ref.numel(), tuple(bad[0].tolist()), float(g[tuple(bad[0])]), float(ref[tuple(bad[0])])))


def _supported(lib, shape, algo):
    N, Cin, H, W, Cout = shape
    assert lib.sstem_conv3x3_algo_supported(N, Cin, H, W, Cout, ALGO[algo]) == 1, "the library refuses %s under %s" % (shape, algo)


def _lib_ksplit(lib, shape, algo):
    N, Cin, H, W, Cout = shape
    extra = lib.sstem_conv3x3_forward_workspace_floats_algo(N, Cin, H, W, Cout, ALGO[algo]) - lib.sstem_conv3x3_packed_floats(Cin, Cout, ALGO[algo])
    assert extra % (N * Cout * H * W) == 0
    return max(1, extra // (N * Cout * H * W))


def _launch_fwd(lib, algo, shape, x, w, flags, bias=None, scale=None, shift=None, act=0, slope=0.0, residual=None, res_scale=1.0,
                in_mask=None, want_mask=False, layout=LAYOUT_NCHW, out=None, out_ptr=None, out_stride=0, pooled=None, pool_kind=0,
                x_word=None, want_out=True):
    """One forward-shaped launch under a split id through the C-ABI.  Returns (out, out_mask, out_amax_word or None, status)."""
    N, Cin, H, W, Cout = shape
    aid = ALGO[algo]
    ws_n = lib.sstem_conv3x3_forward_workspace_floats_algo(N, Cin, H, W, Cout, aid)
    ws = torch.empty(ws_n, device="cuda")
    if out is None and want_out:
        out = torch.full((N, Cout, H, W), NAN, device="cuda")
    optr = out_ptr if out_ptr is not None else _p(out)
    om = torch.zeros(N, Cout, H, W, dtype=torch.bool, device="cuda") if want_mask else None
    ow = torch.zeros(1024, device="cuda")
    xw = (x_word if x_word is not None else _word(lib, x)) if algo == "f16x3" else None
    if in_mask is not None or want_mask:
        assert residual is None and layout == LAYOUT_NCHW and pooled is None and not out_stride
        if algo == "f16x3":
            rc = lib.sstem_conv3x3_forward_scaled_masked_f32(_p(x), _p(xw), _p(in_mask), _p(w), _p(bias), _p(scale), _p(shift), optr, _p(ow),
                                                             _p(om), _p(ws), ws_n, N, Cin, H, W, Cout, flags, act, slope, None)
        else:
            rc = lib.sstem_conv3x3_forward_masked_f32(_p(x), _p(in_mask), _p(w), _p(bias), _p(scale), _p(shift), optr, _p(om), _p(ws), ws_n,
                                                      N, Cin, H, W, Cout, flags, act, slope, None, aid)
            ow = None
    else:
        rc = lib.sstem_conv3x3_forward_scaled_strided_f32(_p(x), _p(xw), _p(w), _p(bias), _p(scale), _p(shift), _p(residual), res_scale, optr,
                                                          _p(ow), _p(ws), ws_n, N, Cin, H, W, Cout, flags, act, slope, None, aid, layout,
                                                          out_stride, _p(pooled), pool_kind)
    torch.cuda.synchronize()
    return out, om, ow, rc


ACTS = ((0, 0.0), (1, 0.0), (2, 0.25))


def _forward_operands(algo, fam, shape, flags, seed):
    """Operands of one forward-shaped call: x dense, the logical weights wl [Cout, Cin, 3, 3] few-hot with one entry of every output
    channel inside the last K chunk; the tensor handed to the library (wl itself, or transposed + flipped for the data-gradient flag);
    pieces, quantum; all on the CPU."""
    N, Cin, H, W, Cout = shape
    last = torch.zeros(Cin, 3, 3, dtype=torch.bool)
    last[(Cin - 1) // 16 * 16:] = True
    x, wl, q = CE.family_operands(algo, fam, (N, Cin, H, W), Cout, (Cin, 3, 3), seed, must_hit=last)
    px, pw = CE.exact_domain(algo, x, wl)
    w_pass = wl.transpose(0, 1).flip(2, 3).contiguous() if flags & 1 else wl
    return x, wl, w_pass, px, pw, q


def _conv_sum_ref(xc, w_pass_c, flags, bias=None):
    """conv + bias in float64 from the tensor the library was given: a convolution, or -- under the transposed flag -- the data
    gradient of the convolution whose [Cout', Cin', 3, 3] weights were passed."""
    ref = CE.conv_dgrad_ref64(xc, w_pass_c) if flags & 1 else CE.conv_ref64(xc, w_pass_c)
    if bias is not None:
        ref = ref + bias.double().view(1, -1, 1, 1)
    return ref


# ---- forward and data gradient -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", IDS)
@pytest.mark.parametrize("row", FWD_ROWS, ids=[r[0] for r in FWD_ROWS])
def test_forward_and_data_gradient_bit_for_bit(row, algo):
    name, shape, (CO, T, V, tail, ks) = row
    N, Cin, H, W, Cout = shape
    lib = _lib()
    _supported(lib, shape, algo)
    want = Inst(CO, 3 if algo == "x6" else 2, V, False, T, tail and algo != "x3", algo == "f16x3", False, False)
    assert fwd_instance(algo, shape) == (want, ks, 1)
    assert _lib_ksplit(lib, shape, algo) == ks
    ri = [r[0] for r in FWD_ROWS].index(name)
    for flags in (0, 1):
        for fi, fam in enumerate(CE.FAMILIES[algo]):
            seed = 1000 * ri + 100 * IDS.index(algo) + 10 * flags + fi
            x, wl, w_pass, px, pw, q = _forward_operands(algo, fam, shape, flags, seed)
            bias, scale, shift, res = CE.epilogue_operands(Cout, (N, Cout, H, W), q, seed, residual=True)
            CE.assert_exactly_summable(CE.forward_terms_abs(px, pw, bias, scale, shift, res), q)
            xc, wc, bc, sc, shc, rc_ = _cuda(x, w_pass, bias, scale, shift, res)
            acc = CE.assert_fp32_number(_conv_sum_ref(xc, wc, flags, bc))
            tag = "%s %s flags=%d family %s" % (name, algo, flags, fam)
            # the whole epilogue in the store (or in the slice-sum launch): folded affine, activation, averaged residual, the bound
            act, slope = ACTS[seed % 3]
            ref = CE.epilogue_ref64(acc, sc, shc, act, slope, rc_, 0.5)
            out, _, ow, rc = _launch_fwd(lib, algo, shape, xc, wc, flags, bc, sc, shc, act, slope, rc_, 0.5)
            sstem_native.check(rc, "split convolution launch")
            _eq(out, ref, tag + " epilogue")
            assert float(ow.max()) == float(ref.abs().max()), tag + ": output bound"
            # no epilogue at all
            plain = CE.assert_fp32_number(_conv_sum_ref(xc, wc, flags))
            out, _, ow, rc = _launch_fwd(lib, algo, shape, xc, wc, flags)
            sstem_native.check(rc, "split convolution launch")
            _eq(out, plain, tag + " plain")
            assert float(ow.max()) == float(plain.abs().max()), tag + ": output bound"
            # the masked instances: input mask, output mask, both
            gen = torch.Generator().manual_seed(seed)
            im = (torch.rand(N, Cin, H, W, generator=gen) > 0.4).cuda()
            xm = torch.where(im, xc, torch.zeros((), device="cuda"))
            xw = _word(lib, xc) if algo == "f16x3" else None
            for mk in MASKS:
                want_m = fwd_instance(algo, shape, masked=True)
                use_in, use_out = mk in ("in", "both"), mk in ("out", "both")
                out, om, ow, rc = _launch_fwd(lib, algo, shape, xc, wc, flags, bc, act=1, in_mask=im if use_in else None, want_mask=use_out,
                                              x_word=xw)
                if want_m is None:                           # the fp16 id has no masked instance behind the dword staging: refused, not wrong
                    assert rc != 0 and algo == "f16x3" and W % 4 != 0
                    continue
                sstem_native.check(rc, tag + " mask " + mk)
                assert want_m[0] == want._replace(M=True)
                mref = torch.relu(CE.assert_fp32_number(_conv_sum_ref(xm if use_in else xc, wc, flags, bc)))
                _eq(out, mref, tag + " mask " + mk)
                if use_out:
                    assert torch.equal(om, mref > 0), tag + " mask " + mk + ": output mask"
                if ow is not None:
                    assert float(ow.max()) == float(mref.abs().max()), tag + " mask " + mk + ": output bound"


@pytest.mark.parametrize("algo", ["x6", "f16x3"])
@pytest.mark.parametrize("row", ONE_HOT_ROWS, ids=[r[0] for r in ONE_HOT_ROWS])
def test_one_hot_weights_on_full_24_bit_inputs(row, algo):
    """A weight tensor with a single 1 per output channel: X6 returns the shifted input bit for bit; F16X3 keeps 22 bits:
    |out - x| <= 2^-22 |x| + 2^-25 bound at every element (include/sstem_conv.h, taken element by element)."""
    name, shape, _ = row
    N, Cin, H, W, Cout = shape
    lib = _lib()
    _supported(lib, shape, algo)
    gen = torch.Generator().manual_seed(FWD_ROWS.index(row))
    x = torch.randn(N, Cin, H, W, generator=gen)
    assert int((x.view(torch.int32) & 0xFF != 0).sum()) > 0.9 * x.numel()      # the low mantissa byte is in use
    wl, _ = CE.few_hot(Cout, (Cin, 3, 3), 1, gen, "ints", [1.0])
    wl = wl.abs()
    for flags in (0, 1):
        w_pass = wl.transpose(0, 1).flip(2, 3).contiguous() if flags else wl
        xc, wc = _cuda(x, w_pass)
        ref = _conv_sum_ref(xc, wc, flags)
        out, _, _, rc = _launch_fwd(lib, algo, shape, xc, wc, flags)
        sstem_native.check(rc, "split convolution launch")
        if algo == "x6":
            _eq(out, ref, "%s one-hot flags=%d" % (name, flags))
        else:
            bound = float(x.abs().max())
            over = (out.double() - ref).abs() - (2.0 ** -22 * ref.abs() + 2.0 ** -25 * bound)
            assert bool((over <= 0).all()), "%s one-hot flags=%d: %d elements outside 2^-22 |x| + 2^-25 bound, worst by %.3g" % (
                name, flags, int((over > 0).sum()), float(over.max()))


def test_tile_walking_stream_bit_for_bit(monkeypatch):
    name, shape = WALK_ROW
    N, Cin, H, W, Cout = shape
    lib = _lib()
    _supported(lib, shape, "f16x3")
    monkeypatch.setenv("SSTEM_SPLIT_WALK", "8"); monkeypatch.setenv("SSTEM_SPLIT_WALK_MIN_WGS", "1")
    assert fwd_instance("f16x3", shape, walk=8, walk_min=1) == (Inst(32, 2, True, False, 32, False, True, True, False), 1, 8)
    assert _cdiv(H, 8) % 8 == 1                                   # a ragged last group of one tile
    for flags in (0, 1):
        for fi, fam in enumerate(CE.FAMILIES["f16x3"]):
            seed = 50000 + 10 * flags + fi
            x, wl, w_pass, px, pw, q = _forward_operands("f16x3", fam, shape, flags, seed)
            bias, scale, shift, res = CE.epilogue_operands(Cout, (N, Cout, H, W), q, seed, residual=True)
            CE.assert_exactly_summable(CE.forward_terms_abs(px, pw, bias, scale, shift, res), q)
            xc, wc, bc, sc, shc, rc_ = _cuda(x, w_pass, bias, scale, shift, res)
            ref = CE.epilogue_ref64(CE.assert_fp32_number(_conv_sum_ref(xc, wc, flags, bc)), sc, shc, 2, 0.25, rc_, 0.5)
            out, _, ow, rc = _launch_fwd(lib, "f16x3", shape, xc, wc, flags, bc, sc, shc, 2, 0.25, rc_, 0.5)
            sstem_native.check(rc, "split convolution launch")
            _eq(out, ref, "%s flags=%d family %s" % (name, flags, fam))
            assert float(ow.max()) == float(ref.abs().max())


def test_store_variants_of_the_fp16_id_bit_for_bit():
    """Row-segment store, store into a channel block of a larger tensor, pooled copies (max and average, with and without the
    full-resolution output): the same sums, stored elsewhere; the pooled copy equals the float64 pooling of the reference."""
    name, shape = STORE_ROW
    N, Cin, H, W, Cout = shape
    lib = _lib()
    _supported(lib, shape, "f16x3")
    assert fwd_instance("f16x3", shape, layout=LAYOUT_ROWSEG)[0] == Inst(32, 2, True, False, 32, False, True, False, False)
    for fi, fam in enumerate(CE.FAMILIES["f16x3"]):
        seed = 60000 + fi
        x, wl, w_pass, px, pw, q = _forward_operands("f16x3", fam, shape, 0, seed)
        bias, scale, shift, _ = CE.epilogue_operands(Cout, (N, Cout, H, W), q, seed)
        CE.assert_exactly_summable(CE.forward_terms_abs(px, pw, bias, scale, shift), q)
        xc, wc, bc, sc, shc = _cuda(x, w_pass, bias, scale, shift)
        ref = CE.epilogue_ref64(CE.assert_fp32_number(_conv_sum_ref(xc, wc, 0, bc)), sc, shc, 2, 0.25)
        TX = _cdiv(W, 64)
        seg = torch.full((N, H, TX, Cout, 64), NAN, device="cuda")
        _, _, ow, rc = _launch_fwd(lib, "f16x3", shape, xc, wc, 0, bc, sc, shc, 2, 0.25, layout=LAYOUT_ROWSEG, out=seg)
        sstem_native.check(rc, "split convolution launch")
        flat = seg.permute(0, 3, 1, 2, 4).reshape(N, Cout, H, TX * 64)
        _eq(flat[..., :W], ref, "row segments, family " + fam)
        assert bool(torch.isnan(flat[..., W:]).all()) and float(ow.max()) == float(ref.abs().max())
        big = torch.full((N, Cout + 5, H, W), NAN, device="cuda")
        _, _, ow, rc = _launch_fwd(lib, "f16x3", shape, xc, wc, 0, bc, sc, shc, 2, 0.25, out=big, out_ptr=big[0, 5].data_ptr(),
                                   out_stride=(Cout + 5) * H * W)
        sstem_native.check(rc, "split convolution launch")
        _eq(big[:, 5:], ref, "channel block, family " + fam)
        assert bool(torch.isnan(big[:, :5]).all()) and float(ow.max()) == float(ref.abs().max())
        for kind in (1, 2):
            pref = CE.assert_fp32_number(CE.pool2x2_ref64(ref, kind), "pooled reference")
            for want_out in (True, False):
                pooled = torch.full((N, Cout, H // 2, W // 2), NAN, device="cuda")
                out, _, ow, rc = _launch_fwd(lib, "f16x3", shape, xc, wc, 0, bc, sc, shc, 2, 0.25, pooled=pooled, pool_kind=kind,
                                             want_out=want_out)
                sstem_native.check(rc, "split convolution launch")
                _eq(pooled, pref, "pooled copy kind %d, family %s" % (kind, fam))
                if want_out:
                    _eq(out, ref, "output beside the pooled copy, family " + fam)
                assert float(ow.max()) == float(ref.abs().max())


# ---- ConvTranspose k3 s2 p1 op1 ------------------------------------------------------------------------------------------------------------
def _convT_operands(algo, fam, shape, seed):
    N, Cin, H, W, C = shape
    x, wl, q = CE.family_operands(algo, fam, (N, Cin, H, W), C, (Cin, 3, 3), seed)
    px, pw = CE.exact_domain(algo, x, wl)
    return x, wl.transpose(0, 1).contiguous(), px, [p.transpose(0, 1).contiguous() for p in pw], q        # weights [Cin, C, 3, 3]


@pytest.mark.parametrize("shape", [CT_TILE_SHAPE, CT_WALK_SHAPE], ids=["per_tile", "walking"])
def test_sub_pixel_conv_transpose_bit_for_bit(shape):
    """SSTEM_LAYOUT_CONVT_PARITY through hipnn: folded affine, LeakyReLU 0.25 and the averaged skip in the pixel-shuffle store."""
    N, Cin, H, W, C = shape
    lib = _lib()
    _supported(lib, (N, Cin, H, W, 4 * C), "f16x3")
    inst, _, cw = fwd_instance("f16x3", (N, Cin, H, W, 4 * C), layout=LAYOUT_CT)
    assert inst == Inst(64, 2, True, False, 32, False, True, shape == CT_WALK_SHAPE, True) and cw == (2 if shape == CT_WALK_SHAPE else 1)
    for fi, fam in enumerate(CE.FAMILIES["f16x3"]):
        seed = 70000 + fi
        x, w, px, pw, q = _convT_operands("f16x3", fam, shape, seed)
        bias, scale, shift, _ = CE.epilogue_operands(C, (1, C, 1, 1), q, seed)
        xc, wc, bc, sc, shc = _cuda(x, w, bias, scale, shift)
        g = torch.Generator(device="cuda").manual_seed(seed)
        step = max(q, 2.0 ** -20)
        res = (torch.randint(-int(1 / step), int(1 / step) + 1, (N, C, 2 * H, 2 * W), device="cuda", generator=g).double() * step).float()
        S = CE.convT_ref64(CE.piece_magnitudes(px).cuda(), CE.piece_magnitudes(pw).cuda()) + (bc.double().abs() + shc.double().abs()).view(1, -1, 1, 1)
        CE.assert_exactly_summable(S + res.double().abs(), q)
        del S
        ref = CE.epilogue_ref64(CE.assert_fp32_number(CE.convT_ref64(xc, wc, bc)), sc, shc, 2, 0.25, res, 0.5)
        m = torch.nn.ConvTranspose2d(Cin, C, 3, stride=2, padding=1, output_padding=1).cuda().requires_grad_(False)
        with torch.no_grad():
            m.weight.copy_(wc); m.bias.copy_(bc)
        with HF.algorithm(HF.ALGO_MFMA_F16X3), torch.no_grad():
            assert HF._convT_subpixel_ok(xc, m.weight, m, False, None)
            got = HF.conv_transpose3x3s2_fused(xc, m.weight, m.bias, sc, shc, HF.ACT_LEAKY, 0.25, owner=m, residual=res, res_scale=0.5)
        _eq(got, ref, "sub-pixel ConvTranspose, family " + fam)
        assert float(HF.amax_word_of(got).max()) == float(ref.abs().max())
        del ref, got, res


def _pixel_grad(nout, N, H, W, seed):
    """A few-hot gradient of small integers, [N, nout, H, W]."""
    g, _ = CE.few_hot_pixels(nout, N, H, W, min(4, N * H * W), torch.Generator().manual_seed(seed + 31), "ints", None)
    return g


@pytest.mark.parametrize("shape", sorted(CONVT_SHAPES, key=lambda s: s[0] * s[1] * s[2] * s[3] * s[4])[:2])
def test_native_fp32_conv_transpose_forward_and_backward_bit_for_bit(shape):
    N, Cin, H, W, C = shape
    for fi, fam in enumerate(CE.FAMILIES["fp32"]):
        seed = 80000 + fi
        x, w, px, pw, q = _convT_operands("fp32", fam, shape, seed)
        bias = CE.epilogue_operands(C, (1, C, 1, 1), q, seed)[0]
        g = _pixel_grad(C, N, 2 * H, 2 * W, seed)
        CE.assert_exactly_summable(CE.convT_ref64(px[0].abs(), pw[0].abs(), bias.abs()), q)
        CE.assert_exactly_summable(CE.convT_dgrad_ref64(g.abs(), pw[0].abs()), q)
        CE.assert_exactly_summable(CE.convT_wgrad_ref64(px[0].abs(), g.abs())[0], q)
        xc, wc, bc, gc = _cuda(x, w, bias, g)
        HF.set_algorithm(HF.ALGO_MFMA)
        xg, wg, bg = xc.clone().requires_grad_(), wc.clone().requires_grad_(), bc.clone().requires_grad_()
        out = HF.conv_transpose3x3s2_fused(xg, wg, bg, None, None, HF.ACT_NONE, 0.0)
        out.backward(gc)
        _eq(out.detach(), CE.assert_fp32_number(CE.convT_ref64(xc, wc, bc)), "ConvTranspose forward, family " + fam)
        _eq(xg.grad, CE.assert_fp32_number(CE.convT_dgrad_ref64(gc, wc)), "ConvTranspose data gradient, family " + fam)
        gw, gb = CE.convT_wgrad_ref64(xc, gc)
        _eq(wg.grad, CE.assert_fp32_number(gw), "ConvTranspose weight gradient, family " + fam)
        _eq(bg.grad, gb, "ConvTranspose bias gradient, family " + fam)


# ---- weight and bias gradient --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", IDS)
@pytest.mark.parametrize("row", WGRAD_ROWS, ids=[r[0] for r in WGRAD_ROWS])
def test_weight_and_bias_gradient_bit_for_bit(row, algo, monkeypatch):
    name, shape, ks = row
    N, Cin, H, W, Cout = shape
    lib = _lib()
    _supported(lib, shape, algo)
    CinP, CoutP, ksplit = wgrad_split_plan(*shape)
    assert ksplit == ks
    ws_n = lib.sstem_conv3x3_wgrad_workspace_floats_algo(N, Cin, H, W, Cout, ALGO[algo])
    assert ws_n == ks * (9 * CoutP * CinP + CoutP)                # the library's plan has the same number of slabs
    ws = torch.empty(ws_n, device="cuda")
    ri = [r[0] for r in WGRAD_ROWS].index(name)
    for fi, fam in enumerate(CE.FAMILIES[algo]):
        seed = 90000 + 1000 * ri + 100 * IDS.index(algo) + fi
        x, g, q = CE.family_operands(algo, fam, (N, Cin, H, W), Cout, None, seed, pixels=(N, H, W))
        gen = torch.Generator().manual_seed(seed)
        mask = torch.rand(N, Cout, H, W, generator=gen) > 0.3
        hit = (g != 0).any(1)
        assert bool(hit[N - 1].any()) and bool(hit[:, H - 1].any()) and bool(hit[:, H - 2].any()) and bool(hit[:, :, W - 1].any())
        assert W <= 32 or (bool(hit[:, :, 31].any()) and bool(hit[:, :, 32].any()))
        px, pg = CE.exact_domain(algo, x, g)
        gw0, _, shift0, _ = CE.epilogue_operands(1, (1,), q, seed)        # (scalars: what the buffers hold before an accumulating call)
        pre_w, pre_b = float(gw0[0]), float(shift0[0])
        S, Sb = CE.conv_wgrad_ref64(CE.piece_magnitudes(px), CE.piece_magnitudes(pg))
        CE.assert_exactly_summable(S + abs(pre_w), q)
        CE.assert_exactly_summable(Sb + abs(pre_b), q)
        xc, gc, mc = _cuda(x, g, mask)
        xw, gword = (_word(lib, xc), _word(lib, gc)) if algo == "f16x3" else (None, None)
        for use_mask in (False, True):
            gm = torch.where(mc, gc, torch.zeros((), device="cuda")) if use_mask else gc
            rw, rb = CE.conv_wgrad_ref64(xc, gm)
            CE.assert_fp32_number(rw); CE.assert_fp32_number(rb)
            for pp in ((1, 0) if algo == "f16x3" else (None,)):
                if pp is not None:
                    monkeypatch.setenv("SSTEM_WGRAD_PINGPONG", str(pp))
                for acc in (0, 1):
                    gw = torch.full((Cout, Cin, 3, 3), pre_w if acc else NAN, device="cuda")
                    gb = torch.full((Cout,), pre_b if acc else NAN, device="cuda")
                    if algo == "f16x3":
                        rc = lib.sstem_conv3x3_backward_weight_scaled_masked_f32(_p(xc), _p(xw), _p(gc), _p(gword), _p(mc) if use_mask else None,
                                                                                 _p(gw), _p(gb), _p(ws), ws_n, N, Cin, H, W, Cout, acc, None)
                    else:
                        rc = lib.sstem_conv3x3_backward_weight_masked_f32(_p(xc), _p(gc), _p(mc) if use_mask else None, _p(gw), _p(gb), _p(ws),
                                                                          ws_n, N, Cin, H, W, Cout, acc, None, ALGO[algo])
                    torch.cuda.synchronize()
                    sstem_native.check(rc, "split convolution launch")
                    tag = "%s %s family %s mask=%s pingpong=%s accumulate=%d" % (name, algo, fam, use_mask, pp, acc)
                    _eq(gw, rw + (pre_w if acc else 0.0), tag + ": weight gradient")
                    _eq(gb, rb + (pre_b if acc else 0.0), tag + ": bias gradient")


# ---- through hipnn: the fp32 ids, and the split ids as the networks reach them ------------------------------------------------------------
def _fp32_case(shape, k, fam, seed, algo="fp32"):
    N, Cin, H, W, Cout = shape
    x, w, q = CE.family_operands(algo, fam, (N, Cin, H, W), Cout, (Cin, k, k), seed)
    px, pw = CE.exact_domain(algo, x, w)
    bias, scale, shift, _ = CE.epilogue_operands(Cout, (1,), q, seed)
    S = CE.conv_ref64(CE.piece_magnitudes(px).cuda(), CE.piece_magnitudes(pw).cuda(), bias.abs().cuda())
    CE.assert_exactly_summable(S + shift.double().abs().cuda().view(1, -1, 1, 1), q)
    return x, w, bias, scale, shift, q


def _hipnn_forward_and_backward(algo, hf_algo, shape, k, fam, seed):
    """conv2d_fused under a forced id: the inference launch with each activation, then a recorded Conv + ReLU and its three gradients
    (the gradient is few-hot small integers, so the data gradient and the weight gradient are inside the id's domain as well)."""
    N, Cin, H, W, Cout = shape
    HF.set_algorithm(hf_algo)
    x, w, bias, scale, shift, q = _fp32_case(shape, k, fam, seed, algo)
    g = _pixel_grad(Cout, N, H, W, seed)
    pg, pw = CE.exact_domain(algo, g, w)
    CE.assert_exactly_summable(CE.conv_dgrad_ref64(CE.piece_magnitudes(pg), CE.piece_magnitudes(pw)), q)
    px, pg = CE.exact_domain(algo, x, g)
    CE.assert_exactly_summable(CE.conv_wgrad_ref64(CE.piece_magnitudes(px), CE.piece_magnitudes(pg), k)[0], q)
    xc, wc, bc, sc, shc, gc = _cuda(x, w, bias, scale, shift, g)
    acc = CE.assert_fp32_number(CE.conv_ref64(xc, wc, bc))
    tag = "%s k=%d %s family %s" % (shape, k, algo, fam)
    for act, slope in ACTS:
        with torch.no_grad():
            out = HF.conv2d_fused(xc, wc, bc, sc, shc, act, slope)
        _eq(out, CE.epilogue_ref64(acc, sc, shc, act, slope), tag + " forward act=%d" % act)
    xg, wg, bg = xc.clone().requires_grad_(), wc.clone().requires_grad_(), bc.clone().requires_grad_()
    out = HF.conv2d_fused(xg, wg, bg, None, None, HF.ACT_RELU, 0.0)
    out.backward(gc)
    _eq(out.detach(), torch.relu(acc), tag + " recorded forward")
    gm = torch.where(acc > 0, gc.double(), torch.zeros((), dtype=torch.float64, device="cuda"))
    _eq(xg.grad, CE.assert_fp32_number(CE.conv_dgrad_ref64(gm, wc)), tag + " data gradient")
    gw, gb = CE.conv_wgrad_ref64(xc, gm, k)
    _eq(wg.grad, CE.assert_fp32_number(gw), tag + " weight gradient")
    _eq(bg.grad, gb, tag + " bias gradient")


@pytest.mark.parametrize("algo", [HF.ALGO_MFMA, HF.ALGO_DIRECT], ids=["mfma", "direct"])
@pytest.mark.parametrize("shape,k", [(s, 3) for s in FP32_SHAPES[:5]] + [((2, 5, 9, 11, 4), 1), ((2, 5, 9, 11, 4), 5)])
def test_fp32_ids_forward_and_backward_bit_for_bit(shape, k, algo):
    for fi, fam in enumerate(CE.FAMILIES["fp32"]):
        seed = 100000 + 10 * FP32_SHAPES.index(shape) + fi if k == 3 else 101000 + 10 * k + fi
        _hipnn_forward_and_backward("fp32", algo, shape, k, fam, seed)


@pytest.mark.parametrize("algo", IDS)
@pytest.mark.parametrize("row", FWD_ROWS[:6], ids=[r[0] for r in FWD_ROWS[:6]])
def test_split_ids_through_hipnn_forward_and_backward_bit_for_bit(row, algo):
    """The same ids as the networks reach them (hipnn's own workspaces, bounds, masks and weight-gradient choice under a forced id), on
    family A: the multi-piece operand is the activation, weights and gradient are one piece."""
    name, shape, _ = row
    _supported(_lib(), shape, algo)
    _hipnn_forward_and_backward(algo, ALGO[algo], shape, 3, "A", 105000 + 10 * FWD_ROWS.index(row) + IDS.index(algo))


def test_fp32_split_k_launch_bit_for_bit():
    shape, slices = min(SPLITK_SHAPES, key=lambda e: e[0][0] * e[0][1] * e[0][2] * e[0][3] * e[0][4] if e[1] > 1 else 1 << 60)
    N, Cin, H, W, Cout = shape
    lib = _lib()
    full = int(lib.sstem_conv3x3_forward_workspace_floats(N, Cin, H, W, Cout))
    assert slices > 1 and full == int(lib.sstem_conv3x3_workspace_floats(Cin, Cout)) + slices * N * Cout * H * W
    for fi, fam in enumerate(CE.FAMILIES["fp32"]):
        x, w, bias, scale, shift, q = _fp32_case(shape, 3, fam, 110000 + fi)
        xc, wc, bc, sc, shc = _cuda(x, w, bias, scale, shift)
        ref = CE.epilogue_ref64(CE.assert_fp32_number(CE.conv_ref64(xc, wc, bc)), sc, shc, 2, 0.25)
        _eq(_c_forward(xc, wc, bc, sc, shc, HF.ACT_LEAKY, 0.25, full), ref, "fp32 MFMA over %d K slices, family %s" % (slices, fam))
        wt = w.transpose(0, 1).flip(2, 3).contiguous().cuda()
        full_t = int(lib.sstem_conv3x3_forward_workspace_floats(N, Cin, H, W, Cout))
        _eq(_c_forward(xc, wt, None, None, None, HF.ACT_NONE, 0.0, full_t, transposed=True), CE.assert_fp32_number(CE.conv_dgrad_ref64(xc, wt)),
            "fp32 MFMA data gradient over K slices, family " + fam)


def test_streaming_small_cout_kernel_bit_for_bit():
    shape = (2, 6, 752, 704, 6)                                   # (the IFNet's first block: an entry of test_conv_gpu.py's streaming list)
    N, Cin, H, W, Cout = shape
    lib = _lib()
    assert lib.sstem_conv3x3_stream_small_supported(N, Cin, H, W, Cout) == 1
    for fi, fam in enumerate(CE.FAMILIES["fp32"]):
        x, w, bias, scale, shift, q = _fp32_case(shape, 3, fam, 120000 + fi)
        xc, wc, bc, sc, shc = _cuda(x, w, bias, scale, shift)
        ref = CE.epilogue_ref64(CE.assert_fp32_number(CE.conv_ref64(xc, wc, bc)), sc, shc, 2, 0.25)
        out = torch.full((N, Cout, H, W), NAN, device="cuda"); ow = torch.zeros(1024, device="cuda")
        rc = lib.sstem_conv3x3_forward_scaled_strided_f32(_p(xc), None, _p(wc), _p(bc), _p(sc), _p(shc), None, 1.0, _p(out), _p(ow), None, 0,
                                                          N, Cin, H, W, Cout, 0, 2, 0.25, None, HF.ALGO_DIRECT, 0, 0, None, 0)
        torch.cuda.synchronize()
        sstem_native.check(rc, "split convolution launch")
        _eq(out, ref, "streaming kernel, family " + fam)
        assert float(ow.max()) == float(ref.abs().max())
