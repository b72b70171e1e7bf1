"""The bf16-operand convolution id (SSTEM_CONV_MFMA_BF16, csrc/conv_bf16_kernels.hip) bit for bit, its roundings included.

Every assertion on a kernel's output is ``torch.equal(got.double(), ref)`` at every element (``_eq`` of test_conv_exact_gpu.py); a bf16
tensor is compared after ``.float()``, which is exact.  The id ROUNDS its operands by contract (include/sstem_conv.h: "rounded to bf16
(RNE)"), so beside exactly summable terms (tests/conv_exact.py: the budget rule) the operands here NEED rounding, with every class of
the rounding present and counted (``needs_rounding``: exact, below half, tie to even downwards, tie to even upwards, above half, carry
into the next binade) -- a randn value is never a tie, so test_conv_bf16_gpu.py cannot tell round-to-nearest-even from
round-half-away.  The reference is the float64 convolution of ``rne_bf16`` of both operands, an integer restatement of the contract.
The bf16 OUTPUT store is held the same way on ``rounding_store_operands`` (8-bit operands whose sums need ten bits), and the bias
gradient against the float64 sum of the UNROUNDED gradient.

The two launchers' plans are restated below (launch_conv3x3_bf16_mfma_io, launch_conv3x3_wgrad_bf16_mfma_in): every row names the
instance it is there for, each case asserts that the restated rules send it there and that the library agrees where it exposes the
plan, and module-level assertions state that the tables reach every one of the 20 + 5 instances the two dispatches can produce
(tests/test_conv_bf16_exact_cpu.py imports them, so they also run without a GPU).  A launch the rules predict to be refused is
asserted as a refusal (rc != 0, nothing written); any other refusal fails its case; nothing skips."""
import collections

import pytest
import torch

import conv_exact as CE
import hipnn.functional as HF
import sstem_native
from test_conv_exact_gpu import ACTS, MASKS, NAN, _cdiv, _cuda, _eq, _lib, _p, _pixel_grad

pytestmark = pytest.mark.gpu

BF = HF.ALGO_MFMA_BF16
FAMS = CE.ROUNDED_FAMILIES
GUARD = 2                                                         # NaN-filled channels on either side of a one-image output


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    monkeypatch.delenv("SSTEM_CONV_KSPLIT", raising=False)
    yield
    HF.set_algorithm(HF.ALGO_AUTO)
    HF.set_bf16_weight_gradient(True)


# ---- the launchers' dispatch, restated ---------------------------------------------------------------------------------------------------
# conv3x3_bf16_mfma<WCO, WR, 2, VEC, INB, OUTB, MASKED>: CO = 32 (WCO, WR = 1, 4) or 64 (2, 2) output channels per workgroup, VEC 16-byte
# staging, INB / OUTB bf16 input / output tensor, MASKED input and / or output mask
BInst = collections.namedtuple("BInst", "CO VEC INB OUTB MASKED")
# conv3x3_wgrad_bf16_mfma<VEC, INB, MASKED>
BWInst = collections.namedtuple("BWInst", "VEC INB MASKED")


def bf16_geom(N, Cin, H, W, Cout):
    """(CO, ncb, ksplit): conv3x3_bf16_co_block and conv3x3_bf16_ksplit = conv_ksplit(tiles * ncb, cdiv(Cin, 16), 512, 2), 32 x 8 tiles."""
    CO = 32 if Cout <= 32 else 64
    ncb, nchunks = _cdiv(Cout, CO), _cdiv(Cin, 16)
    wgs = _cdiv(W, 32) * _cdiv(H, 8) * N * ncb
    ks = 1
    while wgs * ks < 512 and ks < 8 and nchunks % (ks * 2) == 0 and nchunks // (ks * 2) >= 2:
        ks *= 2
    return CO, ncb, ks


def fwd_plan(shape, aligned=True, inb=False, outb=False, in_mask=False, out_mask=False, room=True, entry="io"):
    """(BInst, K slices) of one forward-shaped launch, or None where it is refused.  entry "ex": sstem_conv2d_forward_ex_f32 (fp32
    tensors, no masks); "io": sstem_conv3x3_forward_bf16io[_masked], which asks sstem_conv3x3_bf16io_supported first (W % 4 == 0; a
    bf16 output only where the PLAN is unsplit, whatever the workspace) and wants a 16-byte aligned input for a mask.  room: the
    workspace holds the slices; without it the launch falls back to one."""
    N, Cin, H, W, Cout = shape
    CO, ncb, ks = bf16_geom(*shape)
    if entry == "ex":
        assert not (inb or outb or in_mask or out_mask)
    elif W % 4 != 0 or (outb and ks > 1) or (inb and in_mask) or ((in_mask or out_mask) and not aligned):
        return None
    if not room:
        ks = 1
    vec = W % 4 == 0 and aligned
    masked = in_mask or out_mask
    if (outb and ks > 1) or (inb and not vec) or (masked and not vec) or (in_mask and inb):
        return None
    return BInst(CO, vec, inb, outb, masked), ks


def wgrad_plan(N, Cin, H, W, Cout):
    """(CinP, CoutP, ksplit, tiles per slice, ntiles): wgrad_bf16_plan -- 2-row x 32-column tiles running down 32-column strips, dealt
    in runs to clamp(cdiv(256, blocks), 1, ntiles // 8) workgroups per 64 x 64 channel block."""
    CinP, CoutP = _cdiv(Cin, 64) * 64, _cdiv(Cout, 64) * 64
    ntiles = N * _cdiv(W, 32) * _cdiv(H, 2)
    blocks = (CinP // 64) * (CoutP // 64)
    ks = max(1, min(_cdiv(256, blocks), ntiles // 8))
    return CinP, CoutP, ks, _cdiv(ntiles, ks), ntiles


def wgrad_instance(shape, inb=False, masked=False, aligned=True):
    vec = shape[3] % 4 == 0 and aligned
    if (inb or masked) and not vec:
        return None
    return BWInst(vec, inb, masked)


def _all_fwd_instances():
    """What with_flags(CO == 64, vec, in_bf16, out_bf16, masked) can produce: a bf16 input and the masks exist with the 16-byte staging only."""
    tf = (False, True)
    return {BInst(CO, V, I, O, M) for CO in (32, 64) for V in tf for I in tf for O in tf for M in tf if V or not (I or M)}


def _all_wgrad_instances():
    tf = (False, True)
    return {BWInst(V, I, M) for V in tf for I in tf for M in tf if V or not (I or M)}


# ---- the tables ----------------------------------------------------------------------------------------------------------------------------
# (name, (N, Cin, H, W, Cout), input 16-byte aligned, the instance the row is there for: CO, VEC, K slices)
FWD_ROWS = [
    ("co32_vec_edge", (1, 32, 9, 36, 20), True, (32, True, 1)),    # every tile an edge tile, ragged tile column, one-row tile row, partial channel block
    ("co64_vec", (2, 32, 9, 36, 70), True, (64, True, 1)),         # two channel blocks, the second partial
    ("vec_interior", (1, 16, 17, 96, 32), True, (32, True, 1)),    # tile_interior (bx = by = 1); lean store, full blocks; generic store in the last tile row
    ("vec_interior_cpart", (1, 16, 25, 100, 20), True, (32, True, 1)),     # the lean store with a partial channel block
    ("co32_dword", (1, 32, 9, 37, 20), True, (32, False, 1)),
    ("co64_dword", (1, 32, 9, 37, 70), True, (64, False, 1)),
    ("dword_misaligned", (1, 16, 9, 36, 20), False, (32, False, 1)),       # W % 4 == 0 but the input 4 bytes off: <!VEC, OUTB> through bf16io
    ("dword_misaligned_co64", (1, 16, 9, 36, 70), False, (64, False, 1)),
    ("pad6", (1, 6, 9, 36, 20), True, (32, True, 1)),              # ragged last chunk: less than a half
    ("pad17", (1, 17, 9, 36, 20), True, (32, True, 1)),            # one channel
    ("pad22", (1, 22, 9, 36, 20), True, (32, True, 1)),
    ("pad27", (1, 27, 9, 36, 20), True, (32, True, 1)),            # across the half boundary
    ("pad6_dword", (1, 6, 9, 37, 20), True, (32, False, 1)),
    ("pad17_dword", (1, 17, 9, 37, 20), True, (32, False, 1)),
    ("pad22_dword", (1, 22, 9, 37, 20), True, (32, False, 1)),
    ("pad27_dword", (1, 27, 9, 37, 20), True, (32, False, 1)),
    ("one_chunk", (1, 16, 9, 36, 20), True, (32, True, 1)),        # a K loop that runs once
    ("three_chunks", (1, 48, 9, 36, 20), True, (32, True, 1)),     # an odd chunk count, unsplit
    ("ks2_tail", (1, 51, 9, 36, 20), True, (32, True, 2)),         # two K slices, the ragged chunk in the second
    ("ks4", (2, 128, 16, 16, 64), True, (64, True, 4)),
    ("ks4_odd", (1, 192, 8, 32, 32), True, (32, True, 4)),         # four slices of three chunks (the c + 1 < c_end branch)
    ("ks8", (1, 256, 8, 32, 64), True, (64, True, 8)),
    ("grid12", (3, 16, 9, 36, 20), True, (32, True, 1)),           # 12 workgroups: the XCD re-map with a remainder
]
IO_VARIANTS = ((False, False), (True, False), (False, True), (True, True))        # (bf16 input tensor, bf16 output tensor)
# (input mask, output mask, bf16 input, bf16 output) of the masked entry; an input mask needs an fp32 input
MASK_VARIANTS = [(mk in ("in", "both"), mk in ("out", "both"), False, ob) for mk in MASKS for ob in (False, True)] + \
                [(False, True, True, False), (False, True, True, True)]

# (name, (N, Cin, H, W, Cout), K slices, exponents of the dense gradient: the bias gradient sums N H W UNROUNDED values of up to
# 256 x 2^e in multiples of 2^(e - 2), so the long rows keep e = -2 to stay inside the budget)
WGRAD_ROWS = [
    ("vec", (2, 40, 9, 36, 70), 2, (-2, -1, 0, 1, 2)),             # 16-byte staging, two strips, odd H, two channel blocks in Cout
    ("dword", (1, 24, 9, 37, 33), 1, (-2, -1, 0, 1, 2)),
    ("blocks_2x3", (1, 70, 6, 36, 130), 1, (-2, -1, 0, 1, 2)),     # two input and three output channel blocks: the bias where ib == 0 only
    ("empty_slice", (1, 8, 162, 32, 8), 10, (-2,)),                # 81 tiles, 10 slices of 9: the tenth owns no tile
    ("empty_slice_dword", (1, 8, 162, 30, 8), 10, (-2,)),
    ("one_tile", (1, 20, 2, 20, 24), 1, (-2, -1, 0, 1, 2)),
]
# (bf16 input tensor, gradient mask) of the weight-gradient entries
WGRAD_VARIANTS = ((False, False), (True, False), (False, True), (True, True))


def _fwd_reached():
    got, slices = set(), set()
    for _, shape, aligned, _ in FWD_ROWS:
        r = fwd_plan(shape, aligned, entry="ex")
        got.add(r[0]); slices.add(r[1])
        for inb, outb in IO_VARIANTS:
            r = fwd_plan(shape, aligned, inb, outb)
            if r is not None:
                got.add(r[0])
        for im, om, inb, outb in MASK_VARIANTS:
            r = fwd_plan(shape, aligned, inb, outb, im, om)
            if r is not None:
                got.add(r[0])
    return got, slices


def _wgrad_reached():
    got = set()
    for _, shape, _, _ in WGRAD_ROWS:
        for inb, masked in WGRAD_VARIANTS:
            r = wgrad_instance(shape, inb, masked)
            if r is not None:
                got.add(r)
    return got


_FWD_REACHED, _KSPLITS_REACHED = _fwd_reached()
_WGRAD_REACHED = _wgrad_reached()
# every instance of the two with_flags dispatches is reachable through the C-ABI, and reached: none is listed as unreachable
assert len(_all_fwd_instances()) == 20 and _FWD_REACHED == _all_fwd_instances(), sorted(_all_fwd_instances() - _FWD_REACHED)
assert len(_all_wgrad_instances()) == 5 and _WGRAD_REACHED == _all_wgrad_instances(), sorted(_all_wgrad_instances() - _WGRAD_REACHED)
assert _KSPLITS_REACHED == {1, 2, 4, 8}
assert fwd_plan(FWD_ROWS[6][1], aligned=False, outb=True) == (BInst(32, False, False, True, False), 1)
assert wgrad_plan(*WGRAD_ROWS[3][1])[2:] == (10, 9, 81) and 9 * 9 >= 81          # slice 9 starts at tile 81: it owns none


# ---- helpers -------------------------------------------------------------------------------------------------------------------------------
def _row_id(rows):
    return [r[0] for r in rows]


def _off_by_4_bytes(t):
    """A copy of the fp32 tensor whose storage starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, device=t.device, dtype=torch.float32)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _bf16_tensor(x, aligned=True):
    """A bf16 tensor holding rne_bf16(x) (the cast of a bf16 number is exact), 4 bytes off a 16-byte boundary where asked."""
    r = CE.rne_bf16(x)
    if aligned:
        xb = r.bfloat16()
    else:
        buf = torch.empty(x.numel() + 8, device=x.device, dtype=torch.bfloat16)
        xb = buf[2:2 + x.numel()].view(x.shape)
        xb.copy_(r)
        assert xb.data_ptr() % 16 == 4
    assert torch.equal(xb.float(), r)
    return xb


def _input_mask(x, c0, seed):
    """An input mask of about 60 % ones that drops at least one non-zero element of x in the channels of the last K chunk, in columns
    31 and 32 (a neighbouring tile's halo) and in rows 7 and 8."""
    N, C, H, W = x.shape
    im = (torch.rand(N, C, H, W, generator=torch.Generator().manual_seed(seed)) > 0.4).to(x.device)
    regions = [(slice(c0, C), slice(0, H), slice(0, W)), (slice(0, C), slice(0, H), slice(min(31, W - 1), min(31, W - 1) + 1)),
               (slice(0, C), slice(0, H), slice(min(32, W - 1), min(32, W - 1) + 1)), (slice(0, C), slice(min(7, H - 1), min(7, H - 1) + 1), slice(0, W)),
               (slice(0, C), slice(min(8, H - 1), min(8, H - 1) + 1), slice(0, W))]
    for cs, ys, xs in regions:
        nz = torch.nonzero(x[:, cs, ys, xs])
        assert nz.shape[0] > 0, "the input has no non-zero element in a region the mask must reach"
        n, c, y, xx = nz[nz.shape[0] // 2].tolist()
        im[n, cs.start + c, ys.start + y, xs.start + xx] = False
        assert bool((~im[:, cs, ys, xs] & (x[:, cs, ys, xs] != 0)).any())
    return im


def _place(x, aligned):
    return x if aligned else _off_by_4_bytes(x)


def _lib_ksplit(lib, shape):
    N, Cin, H, W, Cout = shape
    extra = lib.sstem_conv3x3_forward_workspace_floats_algo(N, Cin, H, W, Cout, BF) - lib.sstem_conv3x3_packed_floats(Cin, Cout, BF)
    assert extra % (N * Cout * H * W) == 0
    return max(1, extra // (N * Cout * H * W))


def _launch(lib, shape, x, w, flags, bias=None, scale=None, shift=None, act=0, slope=0.0, entry="ex", out_bf16=False, in_mask=None,
            want_mask=False, ws=None, ws_floats=None):
    """One forward-shaped launch under the bf16 id.  Returns (output, output mask, status).  A one-image output sits between GUARD
    NaN-filled channels, which must stay NaN; a refused launch must leave the output NaN as well."""
    N, Cin, H, W, Cout = shape
    if ws is None:
        ws_n = lib.sstem_conv3x3_forward_workspace_floats_algo(N, Cin, H, W, Cout, BF) if ws_floats is None else ws_floats
        ws = torch.empty(ws_n, device="cuda")
    ws_n = ws.numel()
    g = GUARD if N == 1 else 0
    big = torch.full((N, Cout + 2 * g, H, W), NAN, device="cuda", dtype=torch.bfloat16 if out_bf16 else torch.float32)
    out = big[:, g:g + Cout]
    om = torch.full((N, Cout, H, W), 7, dtype=torch.uint8, device="cuda") if want_mask else None
    inb = 1 if x.dtype == torch.bfloat16 else 0
    if entry == "ex":
        assert not (inb or out_bf16 or want_mask or in_mask is not None)
        rc = lib.sstem_conv2d_forward_ex_f32(_p(x), _p(w), _p(bias), _p(scale), _p(shift), None, 1.0, out.data_ptr(), None, _p(ws), ws_n, N, Cin,
                                             H, W, Cout, 3, 3, 1, 1, flags, act, slope, None, BF)
    elif entry == "io":
        rc = lib.sstem_conv3x3_forward_bf16io(_p(x), inb, _p(w), _p(bias), _p(scale), _p(shift), out.data_ptr(), 1 if out_bf16 else 0, _p(ws),
                                              ws_n, N, Cin, H, W, Cout, flags, act, slope, None)
    else:
        rc = lib.sstem_conv3x3_forward_bf16io_masked(_p(x), inb, _p(in_mask), _p(w), _p(bias), _p(scale), _p(shift), out.data_ptr(),
                                                     1 if out_bf16 else 0, _p(om), _p(ws), ws_n, N, Cin, H, W, Cout, flags, act, slope, None)
    torch.cuda.synchronize()
    if g:
        assert bool(torch.isnan(big[:, :g]).all()) and bool(torch.isnan(big[:, g + Cout:]).all()), "a store outside the output's channels"
    if rc != 0:
        assert bool(torch.isnan(big).all()), "a refused launch wrote to its output"
        assert om is None or bool((om == 7).all()), "a refused launch wrote to its mask"
    return out, om, rc


def _ok(rc, what):
    sstem_native.check(rc, what)


def _operands(fam, shape, flags, seed):
    """x, the logical weights wl [Cout, Cin, 3, 3] (one few-hot entry of every output channel -- under R' one of every image --
    inside the last K chunk), the tensor handed to the library, pieces (= the rounded operands), quantum; all on the CPU."""
    N, Cin, H, W, Cout = shape
    last = torch.zeros(Cin, 3, 3, dtype=torch.bool)
    last[(Cin - 1) // 16 * 16:] = True
    x, wl, q = CE.family_operands("bf16", fam, (N, Cin, H, W), Cout, (Cin, 3, 3), seed, must_hit=last)
    px, pw = CE.exact_domain("bf16", x, wl, rounded=True)
    dense = x if fam == "R" else wl
    assert not torch.equal(CE.rne_bf16(dense), dense)             # the dense operand does need rounding
    w_pass = wl.transpose(0, 1).flip(2, 3).contiguous() if flags & 1 else wl
    return x, wl, w_pass, px, pw, q


def _ref(xc, w_pass_c, flags, bias=None):
    """conv + bias in float64 of the ROUNDED operands, from the tensor the library was given (the data gradient under the flag)."""
    xr, wr = CE.rne_bf16(xc), CE.rne_bf16(w_pass_c)
    ref = CE.conv_dgrad_ref64(xr, wr) if flags & 1 else CE.conv_ref64(xr, wr)
    if bias is not None:
        ref = ref + bias.double().view(1, -1, 1, 1)
    return CE.assert_fp32_number(ref)


def _case(row, flags, fam, ri):
    name, shape, aligned, _ = row
    N, Cin, H, W, Cout = shape
    seed = 200000 + 100 * ri + 10 * flags + FAMS.index(fam)
    x, wl, w_pass, px, pw, q = _operands(fam, shape, flags, seed)
    bias, scale, shift, _ = CE.epilogue_operands(Cout, (N, Cout, H, W), q, seed)
    CE.assert_exactly_summable(CE.forward_terms_abs(px, pw, bias, scale, shift), q)
    xc, wc, bc, sc, shc = _cuda(x, w_pass, bias, scale, shift)
    return seed, _place(xc, aligned), wc, bc, sc, shc, "%s flags=%d family %s" % (name, flags, fam)


def _pack_group(lib, layers):
    """sstem_conv3x3_pack_weights_group_f32 on a table of (weight [Cout, Cin, 3, 3]) layers: [(packed forward, packed transposed)]."""
    table = torch.zeros(len(layers), 16, dtype=torch.int64)
    bufs, first = [], 0
    for i, w in enumerate(layers):
        cout, cin = w.shape[0], w.shape[1]
        f = torch.empty(lib.sstem_conv3x3_packed_floats(cin, cout, BF), device="cuda")
        t = torch.empty(lib.sstem_conv3x3_packed_floats(cout, cin, BF), device="cuda")
        blocks = lib.sstem_conv3x3_pack_group_entry(cin, cout, BF, table[i].data_ptr())
        assert blocks > 0
        table[i, 0], table[i, 1], table[i, 2], table[i, 13] = w.data_ptr(), f.data_ptr(), t.data_ptr(), first
        first += blocks
        bufs.append((f, t))
    tc = table.cuda()
    _ok(lib.sstem_conv3x3_pack_weights_group_f32(tc.data_ptr(), len(layers), first, BF, None), "pack group")
    torch.cuda.synchronize()
    return bufs


# ---- forward and data gradient -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", FWD_ROWS, ids=_row_id(FWD_ROWS))
def test_forward_and_data_gradient_bit_for_bit(row):
    name, shape, aligned, (CO, VEC, ks) = row
    N, Cin, H, W, Cout = shape
    lib = _lib()
    assert lib.sstem_conv3x3_algo_supported(N, Cin, H, W, Cout, BF) == 1
    assert fwd_plan(shape, aligned, entry="ex") == (BInst(CO, VEC, False, False, False), ks)
    assert _lib_ksplit(lib, shape) == ks
    assert lib.sstem_conv3x3_bf16io_supported(N, Cin, H, W, Cout, 0) == (1 if W % 4 == 0 else 0)
    assert lib.sstem_conv3x3_bf16io_supported(N, Cin, H, W, Cout, 1) == (1 if W % 4 == 0 and ks == 1 else 0)
    packed_n = lib.sstem_conv3x3_packed_floats(Cin, Cout, BF)
    ri = _row_id(FWD_ROWS).index(name)
    for fam in FAMS:
        kept = {}
        for flags in (0, 1):
            seed, xc, wc, bc, sc, shc, tag = _case(row, flags, fam, ri)
            act, slope = ACTS[seed % 3]
            ref = CE.epilogue_ref64(_ref(xc, wc, flags, bc), sc, shc, act, slope)
            out, _, rc = _launch(lib, shape, xc, wc, flags, bc, sc, shc, act, slope)
            _ok(rc, tag)
            _eq(out, ref, tag + " epilogue")
            plain, _, rc = _launch(lib, shape, xc, wc, flags)
            _ok(rc, tag)
            _eq(plain, _ref(xc, wc, flags), tag + " plain")
            # residual and bn_partials belong to the fp32 MFMA id: refused here, nothing written
            res = torch.zeros(N, Cout, H, W, device="cuda")
            o2 = torch.full((N, Cout, H, W), NAN, device="cuda")
            ws = torch.empty(lib.sstem_conv3x3_forward_workspace_floats_algo(N, Cin, H, W, Cout, BF), device="cuda")
            rc = lib.sstem_conv2d_forward_ex_f32(_p(xc), _p(wc), None, None, None, _p(res), 1.0, _p(o2), None, _p(ws), ws.numel(), N, Cin, H, W,
                                                 Cout, 3, 3, 1, 1, flags, 0, 0.0, None, BF)
            torch.cuda.synchronize()
            assert rc != 0 and bool(torch.isnan(o2).all())
            # the same launch through the bf16io entry, fp32 in and out
            io, _, rc = _launch(lib, shape, xc, wc, flags, bc, sc, shc, act, slope, entry="io")
            if W % 4 == 0:
                _ok(rc, tag + " bf16io")
                assert fwd_plan(shape, aligned) == (BInst(CO, VEC, False, False, False), ks)
                assert torch.equal(io, out), tag + ": bf16io entry"
            else:
                assert rc != 0 and fwd_plan(shape, aligned) is None
            # K-split rows: a workspace of exactly the packed size runs unsplit -- the same bits
            if ks > 1:
                assert fwd_plan(shape, aligned, room=False, entry="ex") == (BInst(CO, VEC, False, False, False), 1)
                one, _, rc = _launch(lib, shape, xc, wc, flags, bc, sc, shc, act, slope, ws_floats=packed_n)
                _ok(rc, tag + " unsplit")
                assert torch.equal(one, out), tag + ": unsplit launch"
            # prepacked weights: packed by the pack entry in the orientation of this call
            wsp = torch.empty(lib.sstem_conv3x3_forward_workspace_floats_algo(N, Cin, H, W, Cout, BF), device="cuda")
            if flags & 1:                                         # wc is [Cin, Cout, 3, 3]: the weights of a Cout -> Cin layer, its transposed packing
                _ok(lib.sstem_conv3x3_pack_weights_f32(_p(wc), Cout, Cin, BF, None, _p(wsp), None), "pack")
            else:
                _ok(lib.sstem_conv3x3_pack_weights_f32(_p(wc), Cin, Cout, BF, _p(wsp), None, None), "pack")
            pre, _, rc = _launch(lib, shape, xc, wc, flags | 2, bc, sc, shc, act, slope, ws=wsp)
            _ok(rc, tag + " prepacked")
            assert torch.equal(pre, out), tag + ": prepacked launch"
            kept[flags] = (xc, wc, bc, sc, shc, act, slope, out)
        # the group pack on a two-layer table: layer 0 = the forward call's weights, layer 1 = the data-gradient call's
        (f0, _), (_, t1) = _pack_group(lib, [kept[0][1], kept[1][1]])
        for flags, head in ((0, f0), (1, t1)):
            xc, wc, bc, sc, shc, act, slope, out = kept[flags]
            wsp = torch.empty(lib.sstem_conv3x3_forward_workspace_floats_algo(N, Cin, H, W, Cout, BF), device="cuda")
            assert head.numel() == packed_n
            wsp[:packed_n].copy_(head)
            pre, _, rc = _launch(lib, shape, xc, wc, flags | 2, bc, sc, shc, act, slope, ws=wsp)
            _ok(rc, "group-packed launch")
            assert torch.equal(pre, out), "%s flags=%d family %s: group-packed launch" % (name, flags, fam)


# ---- bf16 tensors --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", FWD_ROWS, ids=_row_id(FWD_ROWS))
def test_bf16_input_tensor_bit_for_bit(row):
    """INB: a bf16 tensor holding rne_bf16(x) gives what the fp32-tensor call gives on x, and the reference.  Refused behind the dword
    staging; with a bf16 output refused on a row whose plan is split over K."""
    name, shape, aligned, (CO, VEC, ks) = row
    N, Cin, H, W, Cout = shape
    lib = _lib()
    ri = _row_id(FWD_ROWS).index(name)
    for fam in FAMS:
        for flags in (0, 1):
            seed, xc, wc, bc, sc, shc, tag = _case(row, flags, fam, ri)
            act, slope = ACTS[(seed + 1) % 3]
            xb = _bf16_tensor(xc, aligned)
            want = fwd_plan(shape, aligned, inb=True)
            got, _, rc = _launch(lib, shape, xb, wc, flags, bc, sc, shc, act, slope, entry="io")
            if want is None:
                assert rc != 0 and (W % 4 != 0 or not aligned), tag
            else:
                assert want == (BInst(CO, True, True, False, False), ks)
                _ok(rc, tag + " bf16 input")
                _eq(got, CE.epilogue_ref64(_ref(xc, wc, flags, bc), sc, shc, act, slope), tag + " bf16 input")
                f32, _, rc = _launch(lib, shape, xc, wc, flags, bc, sc, shc, act, slope, entry="io")
                _ok(rc, tag)
                assert torch.equal(got, f32), tag + ": bf16 against fp32 input tensor"
            if ks > 1:                                            # a bf16 output on a K-split row: refused, with any workspace
                for inp in (xc, xb):
                    for wsf in (None, lib.sstem_conv3x3_packed_floats(Cin, Cout, BF)):
                        assert fwd_plan(shape, aligned, inb=inp is xb, outb=True, room=wsf is None) is None
                        _, _, rc = _launch(lib, shape, inp, wc, flags, bc, entry="io", out_bf16=True, ws_floats=wsf)
                        assert rc != 0, tag + ": a bf16 output of a split launch"


STORE_ROWS = [r for r in FWD_ROWS if r[1][3] % 4 == 0 and r[3][2] == 1]
assert {"vec_interior", "co32_vec_edge", "vec_interior_cpart", "dword_misaligned", "dword_misaligned_co64", "co64_vec"} <= set(_row_id(STORE_ROWS))


def _store_case(row, flags, act, ri):
    name, shape, aligned, _ = row
    N, Cin, H, W, Cout = shape
    x, wl, bias, scale, pre, census = CE.rounding_store_operands(shape, 300000 + 10 * ri + flags, act, 0.25)
    if flags & 1:                                                 # the data-gradient spelling passes the weights transposed + flipped
        w_pass = wl.transpose(0, 1).flip(2, 3).contiguous()
        assert torch.equal(CE.conv_dgrad_ref64(x, w_pass), CE.conv_ref64(x, wl))
    else:
        w_pass = wl
    xc, wc, bc, sc = _cuda(x, w_pass, bias, scale)
    return _place(xc, aligned), wc, bc, sc, pre.cuda(), census


@pytest.mark.parametrize("row", STORE_ROWS, ids=_row_id(STORE_ROWS))
def test_bf16_output_store_rounds_to_nearest_even(row):
    """OUTB, alone and with INB: the stored tensor equals rne_bf16 of the float64 epilogue at every element, on values of every
    rounding class, in the lean store (whole tiles), the generic one (edge tiles) and behind the dword staging."""
    name, shape, aligned, (CO, VEC, ks) = row
    N, Cin, H, W, Cout = shape
    lib = _lib()
    ri = _row_id(FWD_ROWS).index(name)
    assert lib.sstem_conv3x3_bf16io_supported(N, Cin, H, W, Cout, 1) == 1
    for flags in (0, 1):
        for act in (0, 2):
            xc, wc, bc, sc, pre, census = _store_case(row, flags, act, ri)
            ref = CE.rne_bf16(pre.float()).double()
            assert int((ref != pre).sum()) > 0.5 * pre.numel()    # the store does round
            tag = "%s flags=%d act=%d" % (name, flags, act)
            f32, _, rc = _launch(lib, shape, xc, wc, flags, bc, sc, None, act, 0.25, entry="io")
            _ok(rc, tag)
            _eq(f32, pre, tag + " fp32 output")
            for inb in (False, True):
                want = fwd_plan(shape, aligned, inb=inb, outb=True)
                xin = _bf16_tensor(xc, aligned) if inb else xc       # (8-bit values: the cast is exact)
                got, _, rc = _launch(lib, shape, xin, wc, flags, bc, sc, None, act, 0.25, entry="io", out_bf16=True)
                if want is None:
                    assert rc != 0 and inb and not aligned
                    continue
                assert want == (BInst(CO, VEC, inb, True, False), 1)
                _ok(rc, tag)
                assert got.dtype == torch.bfloat16
                _eq(got.float(), ref, tag + " bf16 output, bf16 input %s" % inb)


# ---- masks ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", FWD_ROWS, ids=_row_id(FWD_ROWS))
def test_masked_launches_bit_for_bit(row):
    name, shape, aligned, (CO, VEC, ks) = row
    N, Cin, H, W, Cout = shape
    lib = _lib()
    ri = _row_id(FWD_ROWS).index(name)
    c0 = (Cin - 1) // 16 * 16
    for fam in FAMS:
        for flags in (0, 1):
            seed, xc, wc, bc, sc, shc, tag = _case(row, flags, fam, ri)
            act, slope = ACTS[(seed + 2) % 3]
            im = _input_mask(xc, c0, seed)                       # (asserts that it drops elements of the last chunk and of a neighbour's halo)
            assert 0.5 < float(im.float().mean()) < 0.7
            xm = torch.where(im, xc, torch.zeros((), device="cuda"))
            refs = {}
            for use_in in (False, True):
                refs[use_in] = CE.epilogue_ref64(_ref(xm if use_in else xc, wc, flags, bc), sc, shc, act, slope)
            assert not torch.equal(refs[True], refs[False])
            for use_in, use_out, inb, outb in MASK_VARIANTS:
                want = fwd_plan(shape, aligned, inb, outb, use_in, use_out)
                xin = _bf16_tensor(xc, aligned) if inb else xc
                vtag = "%s mask in=%s out=%s bf16 in=%s out=%s" % (tag, use_in, use_out, inb, outb)
                got, om, rc = _launch(lib, shape, xin, wc, flags, bc, sc, shc, act, slope, entry="masked", out_bf16=outb,
                                      in_mask=im if use_in else None, want_mask=use_out)
                if want is None:                                  # the dword staging, a split plan with a bf16 output: refused
                    assert rc != 0 and (not VEC or (outb and ks > 1)), vtag
                    continue
                assert want == (BInst(CO, True, inb, outb, True), ks)
                _ok(rc, vtag)
                ref = refs[use_in]
                if outb:
                    ref = CE.rne_bf16(ref.float()).double()
                _eq(got.float(), ref, vtag)
                if use_out:
                    assert torch.equal(om, (ref > 0).to(torch.uint8)), vtag + ": output mask"
            # an input mask with a bf16 input tensor is refused
            xb = CE.rne_bf16(xc).bfloat16()
            assert fwd_plan(shape, True, inb=True, in_mask=True) is None
            _, _, rc = _launch(lib, shape, xb, wc, flags, bc, entry="masked", in_mask=im)
            assert rc != 0, tag + ": an input mask with a bf16 input"


# ---- weight and bias gradient --------------------------------------------------------------------------------------------------------------
def _launch_wgrad(lib, shape, entry, x, g, mask, acc, pre_w, pre_b, want_bias=True):
    N, Cin, H, W, Cout = shape
    ws_n = lib.sstem_conv3x3_wgrad_workspace_floats_algo(N, Cin, H, W, Cout, BF)
    ws = torch.empty(ws_n, device="cuda")
    gw = torch.full((Cout, Cin, 3, 3), pre_w if acc else NAN, device="cuda")
    gb = torch.full((Cout,), pre_b if acc else NAN, device="cuda") if want_bias else None
    inb = 1 if x.dtype == torch.bfloat16 else 0
    if entry == "ex":
        rc = lib.sstem_conv2d_backward_weight_bias_ex_f32(_p(x), _p(g), _p(gw), _p(gb), _p(ws), ws_n, N, Cin, H, W, Cout, 3, 3, 1, 1, acc, None, BF)
    elif entry == "bf16in":
        rc = lib.sstem_conv3x3_backward_weight_bf16in_ex(_p(x), _p(g), _p(gw), _p(gb), _p(ws), ws_n, N, Cin, H, W, Cout, acc, None)
    else:
        rc = lib.sstem_conv3x3_backward_weight_bf16_masked(_p(x), inb, _p(g), _p(mask), _p(gw), _p(gb), _p(ws), ws_n, N, Cin, H, W, Cout, acc, None)
    torch.cuda.synchronize()
    if rc != 0:
        assert bool(torch.isnan(gw).all()) or acc, "a refused launch wrote to the gradient"
    return gw, gb, rc


@pytest.mark.parametrize("row", WGRAD_ROWS, ids=_row_id(WGRAD_ROWS))
def test_weight_and_bias_gradient_bit_for_bit(row):
    name, shape, ks, exps = row
    N, Cin, H, W, Cout = shape
    lib = _lib()
    CinP, CoutP, ksplit, tpw, ntiles = wgrad_plan(*shape)
    assert ksplit == ks
    assert lib.sstem_conv3x3_wgrad_workspace_floats_algo(N, Cin, H, W, Cout, BF) == ks * (9 * CoutP * CinP + CoutP)
    if name.startswith("empty_slice"):
        assert (ks - 1) * tpw >= ntiles                           # the last slice owns no tile: exact zeros from it
    vec = W % 4 == 0
    ri = _row_id(WGRAD_ROWS).index(name)
    for fi, fam in enumerate(FAMS):
        seed = 400000 + 100 * ri + fi
        x, g, q = CE.family_operands("bf16", fam, (N, Cin, H, W), Cout, None, seed, pixels=(N, H, W), exps=exps)
        px, pg = CE.exact_domain("bf16", x, g, rounded=True)
        hot = ((g if fam == "R" else x) != 0).any(1)              # the few-hot operand's pixels: halo columns, first and last rows, the last tile
        assert bool(hot[N - 1].any()) and bool(hot[:, 0].any()) and bool(hot[:, H - 1].any()) and bool(hot[:, H - 2].any())
        assert bool(hot[:, :, 0].any()) and bool(hot[:, :, W - 1].any()) and bool(hot[N - 1, H - 2:, W - 2:].any())
        assert W <= 32 or (bool(hot[:, :, 31].any()) and bool(hot[:, :, 32].any()))
        gw0, _, shift0, _ = CE.epilogue_operands(1, (1,), q, seed)
        pre_w, pre_b = float(gw0[0]), float(shift0[0])
        S, _ = CE.conv_wgrad_ref64(CE.piece_magnitudes(px), CE.piece_magnitudes(pg))
        CE.assert_exactly_summable(S + abs(pre_w), q)
        qb = q / 4.0                                               # the UNROUNDED gradient: multiples of 2^-4
        CE.assert_quantum(g, qb, "gradient")
        CE.assert_exactly_summable(g.double().abs().sum((0, 2, 3)) + abs(pre_b), qb)
        gen = torch.Generator().manual_seed(seed)
        mask = torch.rand(N, Cout, H, W, generator=gen) > 0.3
        xc, gc, mc = _cuda(x, g, mask)
        xb = CE.rne_bf16(xc).bfloat16()
        for use_mask in (False, True):
            gm = torch.where(mc, gc, torch.zeros((), device="cuda")) if use_mask else gc
            rw, _ = CE.conv_wgrad_ref64(CE.rne_bf16(xc), CE.rne_bf16(gm))
            rb = gm.double().sum((0, 2, 3))                       # from the fp32 values, not from the rounded ones
            CE.assert_fp32_number(rw); CE.assert_fp32_number(rb)
            if fam == "R'" and not use_mask:
                assert not torch.equal(CE.rne_bf16(gm).double().sum((0, 2, 3)), rb)
            entries = [("masked", xc), ("masked", xb)] if use_mask else [("ex", xc), ("bf16in", xb), ("masked", xc)]
            for entry, xin in entries:
                inb = xin.dtype == torch.bfloat16
                want = wgrad_instance(shape, inb, use_mask)
                for acc, want_bias in ((0, True), (1, True), (0, False)):
                    tag = "%s family %s entry %s bf16 input %s mask %s accumulate %d" % (name, fam, entry, inb, use_mask, acc)
                    gw, gb, rc = _launch_wgrad(lib, shape, entry, xin, gc, mc if use_mask else None, acc, pre_w, pre_b, want_bias)
                    if want is None or (entry == "masked" and not vec):      # the dword staging takes fp32 tensors without a mask
                        assert rc != 0 and not vec, tag
                        continue
                    assert want == BWInst(vec, inb, use_mask)
                    _ok(rc, tag)
                    _eq(gw, rw + (pre_w if acc else 0.0), tag + ": weight gradient")
                    if want_bias:
                        _eq(gb, rb + (pre_b if acc else 0.0), tag + ": bias gradient")


# ---- through hipnn -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16_wgrad", [True, False])
def test_conv2d_fused_forward_and_backward_under_the_bf16_id(bf16_wgrad):
    """Conv + ReLU recorded under ALGO_MFMA_BF16 on co64_vec.  With the bf16 weight-gradient kernel: family R, the weight gradient of
    the ROUNDED input.  Switched off: the fp32 kernel's weight gradient of the UNROUNDED operands -- 8-bit operands (family I), on
    which both are exactly summable."""
    shape = FWD_ROWS[1][1]
    N, Cin, H, W, Cout = shape
    fam = "R" if bf16_wgrad else "I"
    seed = 500000 + int(bf16_wgrad)
    x, w, q = CE.family_operands("bf16", fam, (N, Cin, H, W), Cout, (Cin, 3, 3), seed)
    px, pw = CE.exact_domain("bf16", x, w, rounded=fam == "R")
    bias = CE.epilogue_operands(Cout, (1,), q, seed)[0]
    g = _pixel_grad(Cout, N, H, W, seed)
    CE.assert_exactly_summable(CE.forward_terms_abs(px, pw, bias), q)
    CE.assert_exactly_summable(CE.conv_dgrad_ref64(g.abs(), pw[0].abs()), q)
    CE.assert_exactly_summable(CE.conv_wgrad_ref64(px[0].abs(), g.abs())[0], q)
    xc, wc, bc, gc = _cuda(x, w, bias, g)
    xr = CE.rne_bf16(xc)
    assert torch.equal(xr, xc) == (fam == "I")
    acc = CE.assert_fp32_number(CE.conv_ref64(xr, wc, bc))
    HF.set_algorithm(BF)
    HF.set_bf16_weight_gradient(bf16_wgrad)
    for act, slope in ACTS:
        with torch.no_grad():
            out = HF.conv2d_fused(xc, wc, bc, None, None, act, slope)
        _eq(out, CE.epilogue_ref64(acc, None, None, act, slope), "forward act=%d" % act)
    xg, wg, bg = xc.clone().requires_grad_(), wc.clone().requires_grad_(), bc.clone().requires_grad_()
    out = HF.conv2d_fused(xg, wg, bg, None, None, HF.ACT_RELU, 0.0)
    out.backward(gc)
    _eq(out.detach(), torch.relu(acc), "recorded forward")
    gm = torch.where(acc > 0, gc.double(), torch.zeros((), dtype=torch.float64, device="cuda"))
    _eq(xg.grad, CE.assert_fp32_number(CE.conv_dgrad_ref64(gm, wc)), "data gradient")
    gw, gb = CE.conv_wgrad_ref64(xr, gm)
    _eq(wg.grad, CE.assert_fp32_number(gw), "weight gradient")
    _eq(bg.grad, gb, "bias gradient")


def test_the_bf16_tensor_inside_a_block_is_rounded_to_nearest_even(monkeypatch):
    """Conv - LeakyReLU - Conv of one FusedSequential under no_grad hands a bf16 tensor over.  The first convolution's values need
    rounding (rounding_store_operands); the second has ONE weight of 1 per output channel, so the block's output is the inner bf16
    tensor, shifted: rne_bf16 of the float64 epilogue, bit for bit."""
    import torch.nn as nn
    from hipnn import FusedSequential
    N, Cin, H, W = 2, 24, 19, 40
    C1, C2 = 40, 24
    x, w1, b1, _, pre, census = CE.rounding_store_operands((N, Cin, H, W, C1), 600000, 2, 0.25, with_scale=False)
    w2, _ = CE.few_hot(C2, (C1, 3, 3), 1, torch.Generator().manual_seed(600001), "ints", [1.0])
    w2 = w2.abs()
    inner = CE.rne_bf16(pre.float())
    assert int((inner.double() != pre).sum()) > 0.5 * pre.numel()
    ref = CE.conv_ref64(inner, w2)
    seq = FusedSequential(nn.Conv2d(Cin, C1, 3, padding=1), nn.LeakyReLU(0.25), nn.Conv2d(C1, C2, 3, padding=1, bias=False)).cuda().eval()
    with torch.no_grad():
        seq[0].weight.copy_(w1); seq[0].bias.copy_(b1); seq[2].weight.copy_(w2)
    HF.set_algorithm(BF)
    calls = []
    orig = HF.conv3x3_bf16io
    monkeypatch.setattr(HF, "conv3x3_bf16io", lambda *a, **k: (calls.append(k.get("out_bf16")), orig(*a, **k))[1])
    with torch.no_grad():
        got = seq(x.cuda())
    assert calls == [True, False], calls
    _eq(got, ref.cuda(), "block output")


def test_conv_transpose_under_the_bf16_id_bit_for_bit():
    N, Cin, H, W, C = 2, 40, 9, 17, 33
    gen = torch.Generator().manual_seed(700000)
    x, _ = CE.needs_rounding((N, Cin, H, W), gen)
    wl, _ = CE.few_hot(C, (Cin, 3, 3), 6, gen, "ints", [3.0, 1.0, 2.0, 1.0, 3.0, 2.0])
    w = wl.transpose(0, 1).contiguous()                           # [Cin, C, 3, 3]
    bias = CE.epilogue_operands(C, (1,), CE.Q_ROUNDED, 700000)[0]
    xr = CE.rne_bf16(x)
    CE.assert_exactly_summable(CE.convT_ref64(xr.abs(), w.abs(), bias.abs()), CE.Q_ROUNDED)
    xc, wc, bc = _cuda(x, w, bias)
    HF.set_algorithm(BF)
    for act, slope in ACTS:
        with torch.no_grad():
            out = HF.conv_transpose3x3s2_fused(xc, wc, bc, None, None, act, slope)
        ref = CE.epilogue_ref64(CE.assert_fp32_number(CE.convT_ref64(xr.cuda(), wc, bc)), None, None, act, slope)
        _eq(out, ref, "ConvTranspose act=%d" % act)
