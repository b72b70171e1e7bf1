"""CPU checks of tests/conv_exact.py: the float64 references against torch's own operators, every generator against the budget and the
90 % rule, and the proof that the instrument bites -- an emulation of each id's piece arithmetic (torch's .bfloat16() / .half() casts,
fp32 accumulation in a shuffled order) equals the reference on every element with the full product set and differs on more than half
of them under each mutant."""
import pytest
import torch
import torch.nn.functional as F

import conv_exact as CE

RAGGED = [(2, 5, 7, 11, 6), (1, 19, 9, 13, 3)]            # (N, Cin, H, W, Cout)


def _ints(shape, seed):
    return torch.randint(-4, 5, shape, generator=torch.Generator().manual_seed(seed)).double()


# ---- the references ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", RAGGED)
@pytest.mark.parametrize("k", [1, 3, 5])
def test_convolution_references_against_torch(shape, k):
    """Integer operands: float64 sums are exact in any order, so the references EQUAL torch's operators."""
    N, Cin, H, W, Cout = shape
    x, w, b, g = _ints((N, Cin, H, W), 1), _ints((Cout, Cin, k, k), 2), _ints((Cout,), 3), _ints((N, Cout, H, W), 4)
    assert torch.equal(CE.conv_ref64(x, w, b), F.conv2d(x, w, b, padding=k // 2))
    assert torch.equal(CE.conv_dgrad_ref64(g, w), F.conv_transpose2d(g, w, padding=k // 2))
    gw, gb = CE.conv_wgrad_ref64(x, g, k)
    assert torch.equal(gw, torch.nn.grad.conv2d_weight(x, (Cout, Cin, k, k), g, padding=k // 2))
    assert torch.equal(gb, g.sum((0, 2, 3)))


@pytest.mark.parametrize("shape", RAGGED)
def test_transposed_convolution_references_against_torch(shape):
    N, Cin, H, W, Cout = shape
    x, w, b = _ints((N, Cin, H, W), 5).requires_grad_(True), _ints((Cin, Cout, 3, 3), 6).requires_grad_(True), _ints((Cout,), 7)
    g = _ints((N, Cout, 2 * H, 2 * W), 8)
    out = F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=1)
    assert torch.equal(CE.convT_ref64(x.detach(), w.detach(), b), out.detach())
    out.backward(g)
    assert torch.equal(CE.convT_dgrad_ref64(g, w.detach()), x.grad)
    gw, gb = CE.convT_wgrad_ref64(x.detach(), g)
    assert torch.equal(gw, w.grad) and torch.equal(gb, g.sum((0, 2, 3)))


def test_epilogue_and_pooling_references():
    v = _ints((2, 3, 4, 6), 9) * 0.5
    sc, sh, res = torch.tensor([0.5, 1.0, 2.0]), torch.tensor([0.25, -1.0, 0.5]), _ints((2, 3, 4, 6), 10) * 0.25
    got = CE.epilogue_ref64(v, sc, sh, 2, 0.25, res, 0.5)
    want = (F.leaky_relu(v * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1), 0.25) + res) * 0.5
    assert torch.equal(got, want)
    assert torch.equal(CE.pool2x2_ref64(v, 1), F.max_pool2d(v, 2)) and torch.equal(CE.pool2x2_ref64(v, 2), F.avg_pool2d(v, 2))
    with pytest.raises(AssertionError):                  # a stage that is no fp32 number is refused, not rounded
        CE.epilogue_ref64(torch.full((1, 1, 1, 1), 1.0 + 2.0 ** -30, dtype=torch.float64))


# ---- the generators ----------------------------------------------------------------------------------------------------------------------
def test_multi_piece_values_are_the_sum_of_their_pieces_and_populate_every_piece():
    gen = torch.Generator().manual_seed(11)
    for kind, fmt, P in (("bf16x3", "bf16", 3), ("bf16x2", "bf16", 2), ("f16x2", "f16", 2)):
        x, q = CE.multi_piece((4096,), kind, gen)         # (asserts both properties itself; restated here)
        ps = CE.pieces_f16(x) if fmt == "f16" else CE.pieces_bf16(x, P)
        assert torch.equal(sum(p.double() for p in ps), x.double())
        assert all(float((p != 0).double().mean()) >= 0.9 for p in ps)
        CE.assert_quantum(x, q)
    for shift in range(12, 21):                           # the low fp16 piece is populated EVERYWHERE for any of these shifts
        x, _ = CE.multi_piece((4096,), "f16x2", gen, low_shift=shift)
        assert bool((CE.pieces_f16(x)[1] != 0).all())


def test_a_low_term_of_2_to_the_minus_16_leaves_the_third_piece_mostly_empty_and_is_refused():
    gen = torch.Generator().manual_seed(12)
    x, _ = CE.multi_piece((4096,), "bf16x3", gen, low_shift=16, min_populated=0.0, redraw=False)
    empty = float((CE.pieces_bf16(x, 3)[2] == 0).double().mean())
    assert 0.55 <= empty <= 0.8                           # two thirds
    with pytest.raises(AssertionError, match="piece 2"):
        CE.multi_piece((4096,), "bf16x3", gen, low_shift=16, redraw=False)


CASES = [(algo, fam) for algo in ("x6", "x3", "f16x3", "bf16", "fp32") for fam in CE.FAMILIES[algo]]
SMALL = (1, 20, 7, 9, 13)                                  # two K chunks, the last of 4 channels


def _case(algo, fam, seed=0, shape=SMALL, epilogue=False):
    N, Cin, H, W, Cout = shape
    last = torch.zeros(Cin, 3, 3, dtype=torch.bool)
    last[(Cin - 1) // 16 * 16:] = True
    x, w, q = CE.family_operands(algo, fam, (N, Cin, H, W), Cout, (Cin, 3, 3), seed, must_hit=last)
    rounded = fam in CE.ROUNDED_FAMILIES                  # (the bf16 id rounds by contract: the reference is that of the rounded pair)
    px, pw = CE.exact_domain(algo, x, w, rounded=rounded)
    bias, scale, shift, res = CE.epilogue_operands(Cout, (N, Cout, H, W), q, seed, residual=True) if epilogue else (None,) * 4
    S = CE.forward_terms_abs(px, pw, bias, scale, shift, res)
    CE.assert_exactly_summable(S, q)
    ref = CE.assert_fp32_number(CE.conv_ref64(px[0] if rounded else x, pw[0] if rounded else w, bias))
    return x, w, px, pw, q, ref, (bias, scale, shift, res)


@pytest.mark.parametrize("algo,fam", CASES)
def test_every_family_is_inside_the_budget_with_and_without_the_epilogue(algo, fam):
    for seed in range(4):
        x, w, px, pw, q, ref, ep = _case(algo, fam, seed, epilogue=True)
        bias, scale, shift, res = ep
        for act in (0, 1, 2):                              # every stage of every epilogue is an fp32 number
            CE.epilogue_ref64(ref, scale, shift, act, 0.25, res, 0.5)
        assert float(ref.abs().max()) > 0


def test_weight_gradient_pixels_sit_on_the_tile_seams_and_stay_in_the_budget():
    N, Cin, H, W, Cout = 2, 5, 5, 36, 7
    for algo, fam in CASES:
        x, g, q = CE.family_operands(algo, fam, (N, Cin, H, W), Cout, None, 3, pixels=(N, H, W))
        assert g.shape == (N, Cout, H, W)
        px, pg = CE.exact_domain(algo, x, g, rounded=fam in CE.ROUNDED_FAMILIES)
        S, _ = CE.conv_wgrad_ref64(CE.piece_magnitudes(px), CE.piece_magnitudes(pg))
        CE.assert_exactly_summable(S, q)
        CE.assert_fp32_number(CE.conv_wgrad_ref64(x, g)[0])
    hit = ((x if fam == "R'" else g) != 0).any(1)          # the few-hot operand's pixels, [N, H, W]
    assert bool(hit[N - 1].any()) and bool(hit[:, :, 31].any()) and bool(hit[:, :, 32].any()) and bool(hit[:, H - 1].any())
    assert bool(hit[:, 0, 0].any()) and bool(hit[:, :, W - 1].any())


@pytest.mark.parametrize("algo,fam", [("x6", "X"), ("x3", "C"), ("f16x3", "C"), ("bf16", "A")])
def test_a_family_outside_the_domain_is_refused(algo, fam):
    """Three-piece x two-piece under X6 ("X"), two-piece x two-piece under the two-piece ids, a two-piece operand under BF16."""
    gen = torch.Generator().manual_seed(13)
    if fam == "X":
        x, _ = CE.multi_piece((1, 8, 5, 6), "bf16x3", gen)
        w, _ = CE.few_hot(4, (8, 3, 3), 2, gen, "bf16x2")
    else:
        kind = "f16x2" if algo == "f16x3" else "bf16x2"
        x, _ = CE.multi_piece((1, 8, 5, 6), kind, gen)
        w, _ = CE.few_hot(4, (8, 3, 3), 2, gen, kind if fam == "C" else "ints")
        with pytest.raises(CE.OutsideExactDomain):
            CE.family_operands(algo, fam, (1, 8, 5, 6), 4, (8, 3, 3), 0)
    with pytest.raises(CE.OutsideExactDomain):
        CE.exact_domain(algo, x, w)


def test_a_value_more_than_18_binades_below_the_bound_is_refused_under_fp16_pieces():
    x = torch.tensor([3.0, 2.0 ** -20 * 1.001], dtype=torch.float32).view(1, 2, 1, 1)
    with pytest.raises(CE.OutsideExactDomain, match="not the sum"):
        CE.exact_domain("f16x3", x, torch.ones(1, 2, 3, 3))


def test_the_budget_rule_refuses_a_sum_that_is_too_long():
    with pytest.raises(AssertionError, match="exactly summable"):
        CE.assert_exactly_summable(torch.tensor([2.0 ** 23 + 1.0], dtype=torch.float64), 1.0)
    assert CE.assert_exactly_summable(torch.tensor([2.0 ** 23], dtype=torch.float64), 1.0) == 2.0 ** 23


# ---- the instrument bites ----------------------------------------------------------------------------------------------------------------
def _emulate(px, pw, products, seed):
    """sum over `products` (input piece, weight piece) and K = 9 Cin of piece products, fp32 accumulation, ONE shuffled order of all
    the terms of an output element (products and K positions interleaved)."""
    cols = [F.unfold(p, 3, padding=1) for p in px]                               # [N, K, HW]
    mats = [p.reshape(p.shape[0], -1) for p in pw]                               # [Cout, K]
    terms = torch.cat([mats[b][None, :, :, None] * cols[a][:, None, :, :] for a, b in products], dim=2)      # exact fp32 products
    perm = torch.randperm(terms.shape[2], generator=torch.Generator().manual_seed(seed))
    acc = torch.zeros(terms.shape[0], terms.shape[1], terms.shape[3])
    for i in perm.tolist():
        acc = acc + terms[:, :, i]
    N, _, H, W = px[0].shape
    return acc.reshape(N, -1, H, W)


def _mismatch(got, ref):
    return float((got.double() != ref).double().mean())


@pytest.mark.parametrize("algo,fam", CASES)
def test_the_full_product_set_reproduces_the_reference_on_every_element(algo, fam):
    x, w, px, pw, q, ref, _ = _case(algo, fam)
    for seed in (0, 1):
        assert torch.equal(_emulate(px, pw, CE.KEPT[algo][2], seed).double(), ref)


def _populating_family(algo, a, b):
    """The family under which (input piece a) x (weight piece b) is non-zero: A has a multi-piece input, B a multi-piece weight."""
    if a and b:
        return "C"
    return "B" if b else "A"


DROPS = [(algo, prod) for algo in ("x6", "x3", "f16x3") for prod in CE.KEPT[algo][2]]


@pytest.mark.parametrize("algo,prod", DROPS)
def test_mutant_one_product_class_dropped(algo, prod):
    fam = _populating_family(algo, *prod)
    x, w, px, pw, q, ref, _ = _case(algo, fam)
    kept = [p for p in CE.KEPT[algo][2] if p != prod]
    assert _mismatch(_emulate(px, pw, kept, 0), ref) > 0.5


@pytest.mark.parametrize("algo,piece", [("x6", 1), ("x6", 2), ("x3", 1), ("f16x3", 1)])
def test_mutant_a_piece_from_the_neighbouring_channel_in_the_last_chunk(algo, piece):
    x, w, px, pw, q, ref, _ = _case(algo, "A")
    c0 = (x.shape[1] - 1) // 16 * 16
    bad = [p.clone() for p in px]
    bad[piece][:, c0:] = torch.roll(px[piece][:, c0:], 1, dims=1)
    assert _mismatch(_emulate(bad, pw, CE.KEPT[algo][2], 0), ref) > 0.5


@pytest.mark.parametrize("fam", ["A", "B"])
def test_mutant_an_fp16_scale_off_by_one_binade(fam):
    x, w, px, pw, q, ref, _ = _case("f16x3", fam)
    if fam == "A":
        px = CE.pieces_f16(x, scale_binades_off=1)
    else:
        pw = CE.pieces_f16(w, scale_binades_off=1)
    assert _mismatch(_emulate(px, pw, CE.KEPT["f16x3"][2], 0), ref) > 0.5


@pytest.mark.parametrize("fam", ["A", "B"])
def test_mutant_the_third_piece_rounded_instead_of_subtracted(fam):
    x, w, px, pw, q, ref, _ = _case("x6", fam)
    if fam == "A":
        px = CE.pieces_bf16(x, 3, third_from_first_residual=True)
    else:
        pw = CE.pieces_bf16(w, 3, third_from_first_residual=True)
    assert _mismatch(_emulate(px, pw, CE.KEPT["x6"][2], 0), ref) > 0.5


def test_the_two_piece_id_cannot_pass_for_the_three_piece_one():
    """What the 2e-5 tolerance could not tell apart: X3's arithmetic on X6's family A differs on most elements."""
    x, w, px, pw, q, ref, _ = _case("x6", "A")
    assert _mismatch(_emulate(CE.pieces_bf16(x, 2), CE.pieces_bf16(w, 2), CE.KEPT["x3"][2], 0), ref) > 0.5
