"""Pins tests/sepconv_ref64.py (the float64 reference of the every-pixel GPU checks) and proves that its acceptance function bites.

* the three reference functions against oracle/sepconv_numpy.py (sliding windows + einsum: another spelling) to 1e-12 relative,
  at two ragged shapes; strided / blocked-view / bfloat16 coefficient inputs give the same numbers;
* the serial C oracle's fp32 results pass ``assert_within_rounding`` with the derived n (they are honest fp32 evaluations);
* five mutants of a correct fp32 result -- each the kind of slip a tiled kernel makes -- fail it, and the report names where.
"""
import numpy as np
import pytest
import torch

from oracle import sepconv_c, sepconv_numpy
from sepconv_cases import make_case
from sepconv_ref64 import (N_APPLY, N_GRAD, apply_ref64, assert_within_rounding, backward_ref64, forward_ref64,
                           rounding_report)

SHAPES = [(1, 37, 70), (2, 9, 5)]
MUTANT_SHAPE = (1, 70, 37)          # 70 rows: the last three rows of a 64-row tile (61..63) exist


def _t(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]


def _pad(g):
    return np.pad(g, ((0, 0), (0, 0), (25, 25), (25, 25)), mode="edge")


def _apply_case(seed, B, H, W, kind):
    """Two planes [B,1,H,W] and k1v, k1h, k2v, k2h, all float32 numpy."""
    i1, k1v, k1h, _ = make_case(seed, B, 1, H, W, kind)
    i2, k2v, k2h, _ = make_case(seed + 1, B, 1, H, W, kind)
    g1 = np.ascontiguousarray(i1[:, :, 25:25 + H, 25:25 + W])
    g2 = np.ascontiguousarray(i2[:, :, 25:25 + H, 25:25 + W])
    return g1, g2, k1v, k1h, k2v, k2h


def _rel(a, b):
    return float(np.abs(a - b).max()) / float(np.abs(b).max())


# ---- the reference against the numpy restatement -------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("C", [1, 3])
def test_forward_ref64_equals_the_numpy_restatement(B, H, W, C):
    inp, ver, hor, _ = make_case(31 + H, B, C, H, W)
    ref, S = forward_ref64(*_t(inp, ver, hor))
    assert ref.dtype == torch.float64 and S.dtype == torch.float64
    assert _rel(ref.numpy(), sepconv_numpy.forward(inp, ver, hor)) <= 1e-12
    assert _rel(S.numpy(), sepconv_numpy.forward(np.abs(inp), np.abs(ver), np.abs(hor))) <= 1e-12
    assert (S.numpy() >= np.abs(ref.numpy())).all()


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_backward_ref64_equals_the_numpy_restatement(B, H, W):
    inp, ver, hor, grad = make_case(47 + H, B, 3, H, W)
    gv, gh, S_gv, S_gh = backward_ref64(*_t(grad, inp, ver, hor))
    _, rv, rh = sepconv_numpy.backward(grad, inp, ver, hor)
    assert _rel(gv.numpy(), rv) <= 1e-12 and _rel(gh.numpy(), rh) <= 1e-12
    _, av, ah = sepconv_numpy.backward(np.abs(grad), np.abs(inp), np.abs(ver), np.abs(hor))
    assert _rel(S_gv.numpy(), av) <= 1e-12 and _rel(S_gh.numpy(), ah) <= 1e-12


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_apply_ref64_equals_the_numpy_restatement(B, H, W):
    g1, g2, k1v, k1h, k2v, k2h = _apply_case(59 + H, B, H, W, "randn")
    ref, S = apply_ref64(*_t(g1, g2, k1v, k1h, k2v, k2h))
    want = sepconv_numpy.forward(_pad(g2), k2v, k2h) + sepconv_numpy.forward(_pad(g1), k1v, k1h)
    assert ref.shape == (B, 1, H, W) and _rel(ref.numpy(), want) <= 1e-12
    want_S = (sepconv_numpy.forward(_pad(np.abs(g2)), np.abs(k2v), np.abs(k2h))
              + sepconv_numpy.forward(_pad(np.abs(g1)), np.abs(k1v), np.abs(k1h)))
    assert _rel(S.numpy(), want_S) <= 1e-12


def test_apply_ref64_takes_blocked_views_strided_and_bfloat16_coefficients():
    B, H, W = 2, 9, 70                                   # two row segments, the second with 6 live pixels
    g1, g2, *ks = _t(*_apply_case(71, B, H, W, "randn"))
    ref, S = apply_ref64(g1, g2, *ks)

    def blocked(k):                                      # [B,H,T,51,64] as include/sstem_sepconv.h lays it out, padding pixels 0
        T = (W + 63) // 64
        full = torch.zeros(B, 51, H, T * 64)
        full[..., :W] = k
        return full.reshape(B, 51, H, T, 64).permute(0, 2, 3, 1, 4).contiguous()
    views = [blocked(k).permute(0, 3, 1, 2, 4) for k in ks]
    assert all(not v.is_contiguous() for v in views)
    r2, S2 = apply_ref64(g1, g2, *views)
    assert torch.equal(r2, ref) and torch.equal(S2, S)
    strided = [torch.stack((k, k + 1), dim=-1)[..., 0] for k in ks]
    r3, _ = apply_ref64(g1, g2, *strided)
    assert torch.equal(r3, ref)
    kb = [k.to(torch.bfloat16) for k in ks]
    r4, S4 = apply_ref64(g1, g2, *kb)
    r5, S5 = apply_ref64(g1, g2, *[k.float() for k in kb])
    assert torch.equal(r4, r5) and torch.equal(S4, S5) and not torch.equal(r4, ref)


def test_chunking_does_not_change_the_reference(monkeypatch):
    import sepconv_ref64
    inp, ver, hor, grad = _t(*make_case(83, 2, 3, 9, 5))
    whole = forward_ref64(inp, ver, hor) + backward_ref64(grad, inp, ver, hor)
    monkeypatch.setattr(sepconv_ref64, "_CHUNK_PIXELS", 16)          # three rows per forward chunk, one per backward chunk
    parts = forward_ref64(inp, ver, hor) + backward_ref64(grad, inp, ver, hor)
    for a, b in zip(whole, parts):
        assert torch.equal(a, b)


# ---- the C oracle's fp32 results are inside the derived bound ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["randn", "softmax"])
def test_c_oracle_forward_and_gradients_pass_the_rounding_bound(kind):
    B, C, H, W = 1, 3, 37, 70
    inp, ver, hor, grad = make_case(97, B, C, H, W, kind)
    ref, S = forward_ref64(*_t(inp, ver, hor))
    worst = assert_within_rounding(torch.from_numpy(sepconv_c.forward(inp, ver, hor)), ref, S, N_APPLY, "C oracle forward")
    gv, gh, S_gv, S_gh = backward_ref64(*_t(grad, inp, ver, hor))
    _, ov, oh = sepconv_c.backward(grad, inp, ver, hor)
    wv = assert_within_rounding(torch.from_numpy(ov), gv, S_gv, N_GRAD, "C oracle gradVertical")
    wh = assert_within_rounding(torch.from_numpy(oh), gh, S_gh, N_GRAD, "C oracle gradHorizontal")
    print("C oracle, %s coefficients: worst err / (2^-24 S) forward %.2f, gradVertical %.2f, gradHorizontal %.2f" % (kind, worst, wv, wh))


@pytest.mark.parametrize("kind", ["randn", "softmax"])
def test_c_oracle_apply_passes_the_rounding_bound(kind):
    B, H, W = 1, 37, 70
    g1, g2, k1v, k1h, k2v, k2h = _apply_case(101, B, H, W, kind)
    ref, S = apply_ref64(*_t(g1, g2, k1v, k1h, k2v, k2h))
    rep3 = lambda g: np.repeat(_pad(g), 3, axis=1)
    y = sepconv_c.forward(rep3(g2), k2v, k2h) + sepconv_c.forward(rep3(g1), k1v, k1h)          # model_interp.py:90-97, in fp32
    got = y.mean(axis=1, keepdims=True, dtype=np.float32)
    worst = assert_within_rounding(torch.from_numpy(got), ref, S, N_APPLY, "C oracle apply")
    print("C oracle apply, %s coefficients: worst err / (2^-24 S) %.2f" % (kind, worst))


# ---- mutants: each must fail ------------------------------------------------------------------------------------------------------------

def _sep_np(plane, v, h):
    """sum_fy v sum_fx h * window of the replication-padded plane, float64 numpy; returns (sum [B,1,H,W], windows [B,1,H,W,51,51])."""
    win = np.lib.stride_tricks.sliding_window_view(_pad(plane.astype(np.float64)), (51, 51), axis=(2, 3))
    return np.einsum("bcyxij,biyx,bjyx->bcyx", win, v.astype(np.float64), h.astype(np.float64), optimize=True), win


@pytest.fixture(scope="module")
def mutant_case():
    B, H, W = MUTANT_SHAPE
    case = _apply_case(113, B, H, W, "randn")
    ref, S = apply_ref64(*_t(*case))
    g1, g2, k1v, k1h, k2v, k2h = case
    s1, _ = _sep_np(g1, k1v, k1h)
    s2, win2 = _sep_np(g2, k2v, k2h)
    good = (s2 + s1).astype(np.float32)                    # a correct fp32 result: the exact value rounded once
    assert assert_within_rounding(torch.from_numpy(good), ref, S, N_APPLY, "unmutated") <= 1.0
    return case, ref, S, s1, s2, win2


def _fails(got, ref, S):
    t = torch.from_numpy(np.ascontiguousarray(got.astype(np.float32)))
    with pytest.raises(AssertionError) as e:
        assert_within_rounding(t, ref, S, N_APPLY, "mutant")
    print(str(e.value))
    assert "x mod 4, x mod 64, y mod 64, y, H - y, b" in str(e.value)
    return rounding_report(t, ref, S, N_APPLY)


def test_mutant_one_product_of_2601_dropped(mutant_case):
    (g1, g2, k1v, k1h, k2v, k2h), ref, S, s1, s2, win2 = mutant_case
    fy, fx = 17, 40
    got = s1 + s2 - win2[..., fy, fx] * k2v[:, fy:fy + 1].astype(np.float64) * k2h[:, fx:fx + 1].astype(np.float64)
    rep = _fails(got, ref, S)
    assert rep["bad"] >= 0.8 * ref.numel()                 # nearly every pixel: one term of 2 * 2601 is far above 110 roundings


def test_mutant_horizontal_taps_shifted_by_one_in_the_last_lane_of_each_four(mutant_case):
    (g1, g2, k1v, k1h, k2v, k2h), ref, S, s1, s2, _ = mutant_case
    lane3 = (np.arange(ref.shape[3]) % 4 == 3)
    h_bad = np.where(lane3, np.roll(k2h, 1, axis=1), k2h)
    got = s1 + _sep_np(g2, k2v, h_bad)[0]
    rep = _fails(got, ref, S)
    assert rep["first"][3] % 4 == 3 and rep["bad"] <= int(lane3.sum()) * ref.shape[2]


def test_mutant_bottom_replication_clamped_one_row_early(mutant_case):
    (g1, g2, k1v, k1h, k2v, k2h), ref, S, s1, s2, _ = mutant_case
    H = ref.shape[2]
    g2_bad = g2.copy()
    g2_bad[:, :, H - 1] = g2[:, :, H - 2]                  # every read of a row >= H - 1 returns row H - 2
    got = s1 + _sep_np(g2_bad, k2v, k2h)[0]
    rep = _fails(got, ref, S)
    assert rep["first"][2] >= H - 1 - 25                   # only rows whose window reaches row H - 1


def test_mutant_first_images_vertical_taps_in_the_last_rows_of_a_64_row_tile(mutant_case):
    (g1, g2, k1v, k1h, k2v, k2h), ref, S, s1, s2, _ = mutant_case
    rows = (np.arange(ref.shape[2]) % 64 >= 61)[:, None]
    assert rows.sum() == 3
    got = s1 + _sep_np(g2, np.where(rows, k1v, k2v), k2h)[0]
    rep = _fails(got, ref, S)
    assert rep["first"][2] % 64 >= 61 and rep["bad"] <= 3 * ref.shape[3]


def test_mutant_single_element_off_by_200_ulp_of_its_S(mutant_case):
    _, ref, S, s1, s2, _ = mutant_case
    got = (s1 + s2).astype(np.float32).astype(np.float64)
    got[0, 0, 41, 19] += 200 * 2.0 ** -24 * float(S[0, 0, 41, 19])
    rep = _fails(got, ref, S)
    assert rep["bad"] == 1 and rep["first"] == (0, 0, 41, 19) and 190 <= rep["worst"] <= 210


def test_nan_and_inf_fail_the_checker(mutant_case):
    _, ref, S, s1, s2, _ = mutant_case
    for bad in (np.nan, np.inf):
        got = (s1 + s2).copy()
        got[0, 0, 3, 5] = bad
        rep = _fails(got, ref, S)
        assert rep["bad"] == 1 and rep["nonfinite"] == 1 and rep["first"] == (0, 0, 3, 5)
