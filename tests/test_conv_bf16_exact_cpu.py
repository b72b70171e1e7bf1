"""CPU checks behind tests/test_conv_bf16_exact_gpu.py: ``rne_bf16`` against torch's cast on every upper half, the six-class census of
the rounding fixtures, a float32 restatement of the bf16 id (round the operands, exact products, fp32 sums in a shuffled order) equal to
the float64 reference bit for bit on families R, R' and the store fixture, and the proof that the comparison bites: nine mutants of the
restatement, each of which must FAIL it.  The dispatch tables of the GPU file and their "every instance is reached" assertions are
imported, so they run without a GPU as well."""
import pytest
import torch

import conv_exact as CE
import test_conv_bf16_exact_gpu as G
from test_conv_exact_cpu import _emulate, _mismatch

SMALL = (1, 20, 7, 9, 13)                                  # (N, Cin, H, W, Cout): two K chunks, the last of 4 channels
WIDE = (1, 4, 3, 40, 5)                                    # two 32-column tiles


# ---- rne_bf16 ------------------------------------------------------------------------------------------------------------------------------
def test_rne_bf16_equals_torchs_cast_on_every_upper_half():
    hi = torch.arange(65536, dtype=torch.int64)
    for lo in (0, 1, 0x7FFF, 0x8000, 0x8001, 0xFFFF):
        u = (hi << 16) | lo
        x = torch.where(u >= 2 ** 31, u - 2 ** 32, u).to(torch.int32).view(torch.float32)
        got, want = CE.rne_bf16(x), x.bfloat16().float()
        nan = torch.isnan(x)
        assert int(nan.sum()) in (254, 256) and torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.isnan(got), nan)
        assert torch.equal(got[~nan].view(torch.int32), want[~nan].view(torch.int32)), "low half %#x" % lo
        assert bool(((got.view(torch.int32) & 0xFFFF) == 0).all())


def test_the_other_rounding_modes_differ_from_rne_exactly_where_they_should():
    x, census = CE.needs_rounding((200000,), torch.Generator().manual_seed(0))
    r = CE.rne_bf16(x)
    moved = {m: int((CE.rne_bf16(x, m) != r).sum()) for m in ("trunc", "away", "up")}
    assert moved["trunc"] == census["tie_up"] + census["above_half"]              # everything RNE rounds up in magnitude
    assert moved["away"] == census["tie_down"]                                   # ties that RNE sends down
    up = CE.rne_bf16(x, "up")
    tie = (CE._bits(x) & 0xFFFF) == 0x8000
    assert torch.equal(up[~tie], r[~tie]) and bool((up[tie] >= x[tie]).all()) and moved["up"] > 0.4 * int(tie.sum())


# ---- the census ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(200000,), (1, 6, 9, 36), (20, 6, 3, 3), (130,), (2, 70, 9, 36)])
def test_needs_rounding_holds_every_rounding_class(shape):
    x, census = CE.needs_rounding(shape, torch.Generator().manual_seed(5))
    n = x.numel()
    assert census == CE.rounding_census(x) and sum(census[k] for k in CE.CENSUS_CLASSES[:5]) == n
    CE.assert_rounding_census(census, n)
    assert census["carry"] >= 2 and census["carry"] >= 0.002 * n                 # planted where chance leaves a tensor short
    r = CE.rne_bf16(x)
    CE.assert_quantum(r, CE.Q_ROUNDED)
    assert float(r.abs().max()) <= 1024.0 and float(r.abs().min()) >= 32.0
    v = x.double().abs()
    carried = r.double().abs() >= 2.0 ** torch.floor(torch.log2(v) + 1)          # the rounded value left the binade
    assert int(carried.sum()) == census["carry"]


def test_the_census_refuses_randn():
    x = torch.randn(100000, generator=torch.Generator().manual_seed(6))
    census = CE.rounding_census(x)
    assert census["tie_down"] + census["tie_up"] <= 10                            # a randn value is a tie once in 2^16 draws
    with pytest.raises(AssertionError, match="rounding class"):
        CE.assert_rounding_census(census, x.numel())


@pytest.mark.parametrize("act", [0, 2])
def test_the_store_fixture_holds_every_rounding_class_before_the_store(act):
    for shape in ((1, 16, 9, 36, 20), (1, 16, 17, 96, 32)):
        x, w, bias, scale, pre, census = CE.rounding_store_operands(shape, 11, act)
        CE.assert_rounding_census(census, pre.numel())
        assert torch.equal(CE.rne_bf16(x), x) and torch.equal(CE.rne_bf16(w), w)  # nothing rounds on the way in
        per_channel = (w != 0).reshape(w.shape[0], -1).sum(1)
        assert set(per_channel.tolist()) == {2, 3}
        mags = w.abs().reshape(w.shape[0], -1)
        ratios = torch.log2(mags.max(1, keepdim=True).values / mags.clamp_min(2.0 ** -20))
        assert set(ratios[mags != 0].tolist()) <= set(float(j) for j in range(10)) and bool((mags.max(1).values == 1).all())


# ---- the float32 restatement of the id -----------------------------------------------------------------------------------------------------
def _case(fam, shape=SMALL, seed=0):
    N, Cin, H, W, Cout = shape
    last = torch.zeros(Cin, 3, 3, dtype=torch.bool)
    last[(Cin - 1) // 16 * 16:] = True
    x, w, q = CE.family_operands("bf16", fam, (N, Cin, H, W), Cout, (Cin, 3, 3), seed, must_hit=last)
    px, pw = CE.exact_domain("bf16", x, w, rounded=True)
    CE.assert_exactly_summable(CE.forward_terms_abs(px, pw), q)
    return x, w, CE.assert_fp32_number(CE.conv_ref64(px[0], pw[0]))


def _restate(x, w, seed=0, mode_x="rne", mode_w="rne"):
    """The id in float32: both operands rounded, exact products, one shuffled fp32 sum per output element."""
    return _emulate([CE.rne_bf16(x, mode_x)], [CE.rne_bf16(w, mode_w)], [(0, 0)], seed)


@pytest.mark.parametrize("fam", CE.ROUNDED_FAMILIES)
def test_the_restatement_equals_the_float64_reference_in_any_order(fam):
    x, w, ref = _case(fam)
    for seed in range(3):
        assert torch.equal(_restate(x, w, seed).double(), ref)
    wt = w.transpose(0, 1).flip(2, 3).contiguous()                                # the data-gradient spelling of the same sums
    assert torch.equal(CE.conv_dgrad_ref64(CE.rne_bf16(x), CE.rne_bf16(wt)), ref)


def _store(x, w, bias, scale, act, seed, mode="rne"):
    v = _emulate([x], [w], [(0, 0)], seed) + bias.view(1, -1, 1, 1)
    v = v * scale.view(1, -1, 1, 1)
    v = torch.where(v > 0, v, v * 0.25) if act == 2 else v
    return CE.rne_bf16(v, mode)


@pytest.mark.parametrize("act", [0, 2])
def test_the_restated_store_equals_the_rounded_float64_epilogue(act):
    x, w, bias, scale, pre, _ = CE.rounding_store_operands(SMALL, 21, act)
    ref = CE.rne_bf16(pre.float()).double()
    for seed in range(3):
        assert torch.equal(_store(x, w, bias, scale, act, seed).double(), ref)


# ---- the mutants: each must FAIL the comparison ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["trunc", "away", "up"])
def test_mutant_another_rounding_mode(mode):
    """Truncation, round-half-away and round-half-up (towards +infinity) in the staging of the dense operand: R catches it on the
    input side, R' on the weight pack."""
    x, w, ref = _case("R")
    assert _mismatch(_restate(x, w, mode_x=mode), ref) > 0.2
    x, w, ref = _case("R'")
    assert _mismatch(_restate(x, w, mode_w=mode), ref) > 0.2


def test_mutant_the_pack_reads_tap_t_instead_of_8_minus_t_under_the_transposed_flag():
    for fam in CE.ROUNDED_FAMILIES:
        x, w, ref = _case(fam)
        w_pass = w.transpose(0, 1).flip(2, 3).contiguous()                        # what the data-gradient call is given
        good = w_pass.transpose(0, 1).flip(2, 3)                                  # the pack: transpose, reverse the taps
        assert torch.equal(_restate(x, good).double(), ref)
        assert _mismatch(_restate(x, w_pass.transpose(0, 1).contiguous()), ref) > 0.2       # rounds correctly, reads the wrong tap


def test_mutant_the_output_store_truncates():
    x, w, bias, scale, pre, census = CE.rounding_store_operands(SMALL, 21, 2)
    ref = CE.rne_bf16(pre.float()).double()
    assert _mismatch(_store(x, w, bias, scale, 2, 0, "trunc"), ref) > 0.2
    assert _mismatch(_store(x, w, bias, scale, 2, 0, "away"), ref) > 0.02


def test_mutant_the_bias_gradient_summed_from_the_rounded_gradient():
    N, Cin, H, W, Cout = 1, 5, 6, 36, 7
    x, g, q = CE.family_operands("bf16", "R'", (N, Cin, H, W), Cout, None, 3, pixels=(N, H, W))
    CE.assert_exactly_summable(g.double().abs().sum((0, 2, 3)), q / 4.0)
    ref = g.double().sum((0, 2, 3))
    perm = torch.randperm(N * H * W, generator=torch.Generator().manual_seed(0))
    flat = g.permute(1, 0, 2, 3).reshape(Cout, -1)[:, perm]
    acc = torch.zeros(Cout)
    for i in range(flat.shape[1]):
        acc = acc + flat[:, i]
    assert torch.equal(acc.double(), ref)                                          # fp32 sums of the fp32 values: exact
    assert _mismatch(CE.rne_bf16(g).double().sum((0, 2, 3)), ref) == 1.0          # every channel differs


def test_mutant_an_input_mask_ignored_on_the_channels_of_a_ragged_last_chunk():
    x, w, _ = _case("R")
    c0 = (x.shape[1] - 1) // 16 * 16
    im = G._input_mask(x, c0, 7)
    xm = torch.where(im, x, torch.zeros(()))
    ref = CE.conv_ref64(CE.rne_bf16(xm), CE.rne_bf16(w))
    assert torch.equal(_restate(xm, w).double(), ref)
    bad = xm.clone()
    bad[:, c0:] = x[:, c0:]
    assert _mismatch(_restate(bad, w), ref) > 0.2


def test_mutant_one_k_slice_left_out_of_the_slice_sum():
    for fam in CE.ROUNDED_FAMILIES:
        x, w, ref = _case(fam)
        slices = [x.clone(), x.clone()]                                           # two K slices of one chunk each
        slices[0][:, 16:] = 0
        slices[1][:, :16] = 0
        parts = [_restate(s, w) for s in slices]
        assert torch.equal((parts[0] + parts[1]).double(), ref)
        assert _mismatch(parts[0], ref) > 0.2 and _mismatch(parts[1], ref) > 0.2


def _tiled(x, w, wrong_halo):
    """The restatement tile by tile (32 columns): each tile sees its own columns and one halo column on either side; wrong_halo: the
    right halo column holds what the LEFT neighbour's 4-pixel group starts with (x = X0 - 4) instead of x = X0 + 32."""
    N, C, H, W = x.shape
    out = torch.zeros(N, w.shape[0], H, W)
    for X0 in range(0, W, 32):
        X1 = min(X0 + 32, W)
        tile = torch.zeros(N, C, H, 34)
        lo, hi = max(X0 - 1, 0), min(X1 + 1, W)
        tile[..., lo - (X0 - 1):hi - (X0 - 1)] = x[..., lo:hi]
        if wrong_halo and X0 + 32 < W:
            tile[..., 33] = x[..., X0 - 4] if X0 >= 4 else 0.0
        out[..., X0:X1] = _restate(tile, w)[..., 1:1 + X1 - X0]
    return out


def test_mutant_the_right_halo_column_taken_from_the_left_neighbours_group():
    x, w, ref = _case("R", WIDE)
    assert torch.equal(_tiled(x, w, False).double(), ref)
    bad = _tiled(x, w, True)
    assert not torch.equal(bad.double(), ref)
    wrong = torch.nonzero((bad.double() != ref).any(0).any(0).any(0)).reshape(-1).tolist()
    assert wrong == [31]                                                          # one column of one tile: what a tolerance on max|ref| lets through


# ---- the restated dispatch -----------------------------------------------------------------------------------------------------------------
def test_the_tables_reach_every_instance_of_both_dispatches():
    assert G._FWD_REACHED == G._all_fwd_instances() and len(G._FWD_REACHED) == 20
    assert G._WGRAD_REACHED == G._all_wgrad_instances() and len(G._WGRAD_REACHED) == 5
    assert G._KSPLITS_REACHED == {1, 2, 4, 8}


def test_the_restated_forward_rules():
    for name, shape, aligned, (CO, VEC, ks) in G.FWD_ROWS:
        N, Cin, H, W, Cout = shape
        assert G.bf16_geom(*shape)[::2] == (CO, ks), name
        assert G.fwd_plan(shape, aligned, entry="ex") == (G.BInst(CO, VEC, False, False, False), ks), name
        assert VEC == (W % 4 == 0 and aligned)
        assert G.fwd_plan(shape, aligned, room=False, entry="ex")[1] == 1                         # no room for the slices: one
        assert (G.fwd_plan(shape, aligned, outb=True) is None) == (W % 4 != 0 or ks > 1)          # a bf16 output meets K slices
        assert (G.fwd_plan(shape, aligned, inb=True) is None) == (not VEC)                        # a bf16 input or a mask meets the dword staging
        assert (G.fwd_plan(shape, aligned, out_mask=True) is None) == (not VEC)
        assert G.fwd_plan(shape, aligned, inb=True, in_mask=True) is None                         # an input mask meets a bf16 input
    rows = dict((r[0], r) for r in G.FWD_ROWS)
    assert G.fwd_plan(rows["dword_misaligned"][1], False, outb=True)[0] == G.BInst(32, False, False, True, False)
    assert G.fwd_plan(rows["dword_misaligned_co64"][1], False, outb=True)[0] == G.BInst(64, False, False, True, False)
    # the tiles the rows are there for (32 x 8 tiles; tile_interior: Y0 >= 1, Y0 + 9 <= H, X0 >= 4, X0 + 36 <= W; whole: Y0 + 8 <= H, X0 + 32 <= W)
    def tiles(shape, pred):
        _, _, H, W, _ = shape
        return [(X0 // 32, Y0 // 8) for Y0 in range(0, H, 8) for X0 in range(0, W, 32) if pred(X0, Y0, H, W)]
    interior = lambda X0, Y0, H, W: Y0 >= 1 and Y0 + 9 <= H and X0 >= 4 and X0 + 36 <= W         # noqa: E731
    whole = lambda X0, Y0, H, W: Y0 + 8 <= H and X0 + 32 <= W                                     # noqa: E731
    assert tiles(rows["co32_vec_edge"][1], interior) == [] and tiles(rows["vec_interior"][1], interior) == [(1, 1)]
    assert len(tiles(rows["vec_interior"][1], whole)) == 6 and len(tiles(rows["vec_interior_cpart"][1], whole)) == 9
    assert len(tiles(rows["vec_interior_cpart"][1], interior)) == 4 and rows["vec_interior_cpart"][1][4] % 32 != 0
    assert G._cdiv(192, 16) // G.bf16_geom(*rows["ks4_odd"][1])[2] == 3                           # slices of three chunks
    N, Cin, H, W, Cout = rows["grid12"][1]
    assert G._cdiv(W, 32) * G._cdiv(H, 8) * N == 12 and 12 % 8 != 0


def test_the_restated_weight_gradient_rules():
    for name, shape, ks, exps in G.WGRAD_ROWS:
        CinP, CoutP, ksplit, tpw, ntiles = G.wgrad_plan(*shape)
        assert ksplit == ks, name
        assert G.wgrad_instance(shape) == G.BWInst(shape[3] % 4 == 0, False, False)
        N, _, H, W, _ = shape
        assert N * H * W * 256.0 * 2.0 ** max(exps) <= 2.0 ** 23 * 2.0 ** (min(exps) - 2) * 16 or exps == (-2, -1, 0, 1, 2)
    rows = dict((r[0], r) for r in G.WGRAD_ROWS)
    for name in ("empty_slice", "empty_slice_dword"):
        _, _, ks, tpw, ntiles = G.wgrad_plan(*rows[name][1])
        assert (ks, tpw, ntiles) == (10, 9, 81) and (ks - 1) * tpw >= ntiles                     # the tenth slice owns no tile
    assert G.wgrad_plan(*rows["one_tile"][1])[4] == 1
    assert G.wgrad_plan(*rows["blocks_2x3"][1])[:2] == (128, 192)
    assert G.wgrad_instance(rows["dword"][1], masked=True) is None and G.wgrad_instance(rows["dword"][1], inb=True) is None
