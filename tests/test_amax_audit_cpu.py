"""The Python rules that carry amax words past the launches (hipnn/functional.py: amax_word_of, tag_amax, hand_on_amax, tag_concat_amax,
tag_sum_amax), the audit that holds them (tests/amax_audit.py), and the count behind the one rule that is not exact: bilinear
up-sampling.  None of this needs a device.

The up-sampling count.  hipnn hands x's word on to the up-sampled tensor ("convex: x's bound holds").  In float32 that is not literally
true: lerp2(w0, a, w1, b) = fma(w1, b, rn(w0 a)) with w0 = rn(1 - w1) rounds three times, and l0 + l1 can be 1 + 2^-25 where the
source coordinate lies below 1.  tests/amax_audit.py counts (1 + u)^6 <= 1 + 7 u for the two lerp2 of an output (N_UP_AMAX = 7); the
search below runs the kernels' arithmetic operation by operation (tests/stream_ref64.py ``upsample2x_twin32``) over heights and widths
1 .. 64 on constant and alternating planes, finds how far an output really exceeds the largest input, and holds that to the count."""
import numpy as np
import pytest
import torch

import amax_audit as AA
import hipnn.functional as HF
import stream_ref64 as R

U = 2.0 ** -24


def _word(bound, slot=7):
    w = torch.zeros(1024)
    w[slot] = bound
    return w


def _tagged(t, slot=7):
    return HF.tag_amax(t, _word(float(t.abs().max()), slot))


# ---- the rules ------------------------------------------------------------------------------------------------------------------------------
def test_a_word_goes_stale_with_the_tensors_version():
    t = _tagged(torch.randn(3, 4))
    w = HF.amax_word_of(t)
    assert w is not None and float(w.max()) == float(t.abs().max())
    t.mul_(2.0)                                                  # an in-place edit: the pair is stale, the consumer measures
    assert HF.amax_word_of(t) is None
    _tagged(t)
    assert HF.amax_word_of(t) is not None
    t[0, 0] = 100.0                                              # an indexed store bumps the version as well
    assert HF.amax_word_of(t) is None
    assert HF.amax_word_of(torch.randn(2)) is None               # never tagged


def test_views_read_their_bases_word_and_share_its_version():
    base = _tagged(torch.randn(2, 6, 4, 4))
    w = HF.amax_word_of(base)
    for view in (base[:, 2:4], base[1], base.view(12, 16), base.transpose(2, 3), base[:, ::2]):
        assert HF.amax_word_of(view) is w and float(view.abs().max()) <= float(w.max())
    v = base[:, :3]
    v.zero_()                                                    # an edit THROUGH a view: base and every view are stale
    assert HF.amax_word_of(base) is None and HF.amax_word_of(base[:, 3:]) is None and HF.amax_word_of(v) is None
    own = _tagged(base[:, 3:])                                   # a view with a word of its own
    assert HF.amax_word_of(own) is not None and HF.amax_word_of(base) is None
    base.add_(1.0)
    assert HF.amax_word_of(own) is None                          # (views share their base's version counter)
    assert HF.amax_word_of(base.clone()) is None                 # a copy is a new tensor: no word


def test_concatenation_is_tagged_only_when_every_part_is():
    a, b, c = _tagged(torch.randn(1, 2, 3, 3), 1), _tagged(torch.randn(1, 3, 3, 3) * 5, 900), torch.randn(1, 1, 3, 3) * 50
    cat = HF.tag_concat_amax(torch.cat([a, b], 1), a, b)
    w = HF.amax_word_of(cat)
    assert w is not None and float(w.max()) == float(cat.abs().max()) and float(w[1]) == float(a.abs().max()) and float(w[900]) == float(b.abs().max())
    assert HF.amax_word_of(HF.tag_concat_amax(torch.cat([a, b, c], 1), a, b, c)) is None      # one untagged part: measured by the consumer
    a.neg_()
    assert HF.amax_word_of(HF.tag_concat_amax(torch.cat([a, b], 1), a, b)) is None            # one stale part


@pytest.mark.parametrize("scale", [1.0, 0.5, -0.5, -1.0, 1.0 / 3.0, -0.7, 1e-3, 3.0e5, 2.0 ** -30])
def test_sum_rule_arithmetic(scale):
    """s = (a + b) * scale in float32 against the word max(wa, wb) * (2 |scale|): fl(fl(a + b) fl(scale)) <= fl(2 M fl(scale)) by the
    monotonicity of rounding, and 2 fl32(s) = fl32(2 s) makes the word that very number when |a| = |b| = M -- the bound is attained."""
    g = torch.Generator().manual_seed(5)
    s32 = torch.tensor(scale, dtype=torch.float32)
    assert float(2.0 * s32) == float(torch.tensor(2.0 * scale, dtype=torch.float32))
    for M in (1.0, 1.9999999, 3.0e-5, 7.1e6, float(torch.rand((), generator=g)) + 1.0):
        a = _tagged((torch.rand(4, 5, generator=g) * 2 - 1) * M, 3)
        a[0, 0] = M; _tagged(a, 3)
        b = _tagged(torch.rand(4, 5, generator=g) * M, 4)
        b[0, 0] = M; _tagged(b, 4)
        s = (a + b) * scale
        HF.tag_sum_amax(s, a, b, scale)
        w = HF.amax_word_of(s)
        M32 = float(torch.tensor(M, dtype=torch.float32))
        assert float(w.max()) == float(torch.tensor(M32, dtype=torch.float32) * (2.0 * abs(float(s32))))
        assert float(s.abs().max()) == float(w.max()), "the sum of two maxima attains the bound: %r vs %r" % (float(s.abs().max()), float(w.max()))
    u = torch.randn(3)
    assert HF.amax_word_of(HF.tag_sum_amax(u + a[0, :3], u, a[0, :3])) is None             # one untagged operand


# ---- the audit itself -------------------------------------------------------------------------------------------------------------------
def test_the_audit_records_rules_callers_and_ratios(monkeypatch):
    with AA.audit(monkeypatch) as a:
        x = torch.randn(2, 3, 4, 4)
        HF.tag_amax(x, _word(4.0 * float(x.abs().max())))
        y = HF.hand_on_amax(x, x[:, :, ::2, ::2].contiguous())
        cat = HF.tag_concat_amax(torch.cat([x, x], 1), x, x)
        s = HF.tag_sum_amax((x + x) * 0.5, x, x, 0.5)
        for t in (y, cat, s, x[:, 1]):
            assert HF.amax_word_of(t) is not None
    a.assert_clean()
    assert set(a.rules) == {"produced:test_the_audit_records_rules_callers_and_ratios", "hand_on:test_the_audit_records_rules_callers_and_ratios",
                            "concat", "sum"}, a.rules
    assert 4.0 <= a.max_ratio < 64.0 and len(a) >= 8
    assert HF.amax_word_of.__name__ == "amax_word_of"            # the wrappers are gone


# ---- mutants: rules that are wrong fail the audit --------------------------------------------------------------------------------------------
def _audited(monkeypatch, build, **kw):
    with AA.audit(monkeypatch, **kw) as a:
        for t in build():
            assert HF.amax_word_of(t) is not None
    return a


def _fails(monkeypatch, build, control, **kw):
    a = _audited(monkeypatch, control, **kw)
    a.assert_clean()
    assert len(a) > 0
    a = _audited(monkeypatch, build, **kw)
    assert a.violations, "the mutant passed the audit:\n" + a.report()
    with pytest.raises(AssertionError):
        a.assert_clean()
    return a


def test_mutant_a_rule_that_tags_half_the_word(monkeypatch):
    x = torch.randn(2, 3, 8, 8)
    _fails(monkeypatch, lambda: [HF.tag_amax(x.clone(), _word(float(x.abs().max()) / 2))], lambda: [_tagged(x.clone())])
    # ... and by the last bit
    _fails(monkeypatch, lambda: [HF.tag_amax(x.clone(), _word(float(torch.nextafter(x.abs().max(), torch.tensor(0.0)))))], lambda: [_tagged(x.clone())])


def test_mutant_a_hand_on_across_an_in_place_edit(monkeypatch):
    def build(edit):
        src = _tagged(torch.randn(2, 3, 8, 8))
        dst = src[:, :, ::2, ::2].contiguous()
        if edit:
            dst.mul_(3.0)                                        # the selection is edited BEFORE the word is handed on
        return [HF.hand_on_amax(src, dst)]
    _fails(monkeypatch, lambda: build(True), lambda: build(False))


def test_mutant_a_concatenation_bound_taken_from_one_half(monkeypatch):
    a, b = _tagged(torch.randn(1, 2, 4, 4)), _tagged(torch.randn(1, 2, 4, 4) * 9.0)

    def mutant():
        return [HF.tag_amax(torch.cat([a, b], 1), HF.amax_word_of(a))]
    _fails(monkeypatch, mutant, lambda: [HF.tag_concat_amax(torch.cat([a, b], 1), a, b)])


def test_mutant_a_sum_bound_without_the_factor_two(monkeypatch):
    a = _tagged(torch.rand(1, 2, 4, 4) + 1.0)
    b = _tagged(a.clone())

    def mutant():
        return [HF.tag_amax((a + b) * 0.75, torch.maximum(HF.amax_word_of(a), HF.amax_word_of(b)) * 0.75)]
    _fails(monkeypatch, mutant, lambda: [HF.tag_sum_amax((a + b) * 0.75, a, b, 0.75), HF.tag_sum_amax((a + b) * -0.5, a, b, -0.5)])


def test_mutant_times_four_in_place_of_times_sixteen(monkeypatch):
    """The up-sampling backward gathers, per source pixel, the weights of the outputs that read it (hipnn/functional.py: 16 x the
    gradient's bound).  On a 3 x 3 source plane the centre pixel is read by 4 x 4 outputs with weights (0.4, 0.8, 0.8, 0.4) per axis:
    a constant gradient puts 2.4^2 = 5.76 times its value there -- x4 fails, x16 holds.  Over all plane sizes a pixel is read by at
    most 4 outputs per axis, each with a weight of at most 1: 16 is a bound, and the sums stay below 9."""
    g = _tagged(torch.full((2, 6, 6), 0.37))
    ref, _ = R.upsample2x_backward_ref64(g, 3, 3)
    gin = ref.float()
    assert abs(float(gin.max()) / 0.37 - 5.76) < 1e-5 and int((R.axis_matrix(3) > 0).sum(0).max()) == 4
    _fails(monkeypatch, lambda: [HF.tag_amax(gin.clone(), HF.amax_word_of(g) * 4.0)], lambda: [HF.tag_amax(gin.clone(), HF.amax_word_of(g) * 16.0)])
    assert max(int((R.axis_matrix(n) > 0).sum(0).max()) for n in range(1, 65)) <= 4
    worst = max(float((R.axis_matrix(n).sum(0)).max()) for n in range(1, 65))
    assert 4.0 < worst ** 2 <= 9.0, worst                        # no plane size gathers more: the factor has room


# ---- bilinear up-sampling: how far an output exceeds the largest input -------------------------------------------------------------------------
def _line(n, a, b):
    """The 2n outputs of one axis of n source pixels for the line that alternates a, b, a, ... (float64 arrays of float32 values,
    trailing axes broadcast): lerp2(l0, v[i0], l1, v[i1])."""
    i0, i1, l0, l1 = [t.numpy() for t in R.axis_coords(n)]
    l0, l1 = l0.astype(np.float64), l1.astype(np.float64)
    shape = (-1,) + (1,) * a.ndim
    va = np.where((i0 % 2 == 0).reshape(shape), a, b)
    vb = np.where((i1 % 2 == 0).reshape(shape), a, b)
    return R.lerp2_32(l0.reshape(shape), va, l1.reshape(shape), vb)


@pytest.fixture(scope="module")
def upsampling_excess():
    """Worst (|output| - M) / (2^-24 M) over heights and widths 1 .. 64.  Constant planes: a plane of value M becomes, row by row, the
    line f_W(M), and every column of that the line f_H(value) -- the two passes act element by element, so every (H, W, M) is covered by
    running f_W over the M's and f_H over the distinct (value, M) pairs that come out.  2000 random mantissas and the binade's edges.
    Alternating planes (a checkerboard of +-M; columns, or rows, that alternate M and its predecessor) run
    the same way, at the M the constant search found worst."""
    rng = np.random.default_rng(7)
    Ms = np.concatenate([rng.uniform(1.0, 2.0, 2000).astype(np.float32),
                         np.array([1.0, 1.0000001, 1.5, np.nextafter(np.float32(2.0), np.float32(0.0))], dtype=np.float32)]).astype(np.float64)
    lines = {n: _line(n, Ms, Ms) for n in range(1, 65)}          # [2n, K]
    one_axis = max(float(((lines[n] - Ms) / (Ms * U)).max()) for n in lines)
    # distinct (value, M) pairs: a value lies a few float32 steps from its M, so (index of M, steps) is a small integer key
    m_bits = Ms.astype(np.float32).view(np.int32).astype(np.int64)
    keys = []
    for n in lines:
        steps = lines[n].astype(np.float32).view(np.int32).astype(np.int64) - m_bits
        assert int(np.abs(steps).max()) < 512
        keys.append((np.arange(len(Ms), dtype=np.int64) * 1024 + steps + 512).reshape(-1))
    keys = np.unique(np.concatenate(keys))
    pm = Ms[keys // 1024]
    pairs = np.stack([(m_bits[keys // 1024] + keys % 1024 - 512).astype(np.int32).view(np.float32).astype(np.float64), pm], 1)
    worst, where = 0.0, None
    for H in range(1, 65):
        out = _line(H, pairs[:, 0], pairs[:, 0])
        ex = (np.abs(out) - pairs[:, 1]) / (pairs[:, 1] * U)
        if float(ex.max()) > worst:
            k = np.unravel_index(int(np.argmax(ex)), ex.shape)
            worst, where = float(ex.max()), (H, float(pairs[k[1], 1]))
    # the width at which that M exceeds, for the record (and for the GPU comparison with the kernels)
    Mw = np.float64(np.float32(where[1]))
    W_at = max(range(1, 65), key=lambda n: float(_line(n, Mw, Mw).max()))
    # alternating planes at that M, as (even row, odd row) lines per width: a checkerboard of +-M; columns that alternate M and its
    # predecessor; rows that alternate the predecessor and M.  The vertical pass again runs over the distinct pairs.
    Mp = np.float64(np.nextafter(np.float32(Mw), np.float32(0.0)))
    rows = []
    for n in range(1, 65):
        chk, col = _line(n, Mw, -Mw), _line(n, Mw, Mp)
        rows += [np.stack([chk, -chk], 1), np.stack([col, col], 1), np.stack([_line(n, Mp, Mp), _line(n, Mw, Mw)], 1)]
    ap = np.unique(np.concatenate(rows), axis=0)
    alt = max(float(((np.abs(_line(H, ap[:, 0], ap[:, 1])) - Mw) / (Mw * U)).max()) for H in range(1, 65))
    return {"one_axis": one_axis, "constant": worst, "at": (where[0], W_at, float(Mw)), "alternating": alt}


def test_the_twin_is_the_contract():
    """The float32 twin against the float64 reference of the same contract, within the forward kernels' own bound (N_UP)."""
    g = torch.Generator().manual_seed(3)
    for shape in ((3, 7, 10), (2, 1, 6), (2, 64, 2), (1, 33, 64)):
        x = torch.randn(shape, generator=g)
        ref, S = R.upsample2x_ref64(x)
        R.assert_within_rounding(torch.from_numpy(R.upsample2x_twin32(x.numpy())), ref, S, R.N_UP, "twin %s" % (shape,))
    c = np.full((1, 5, 8), 0.3, dtype=np.float32)
    assert np.array_equal(R.upsample2x_twin32(c)[..., ::2, :][..., 0], np.full((1, 5), 0.3, dtype=np.float32))      # weight (1, 0): the value itself


def test_upsampling_exceeds_its_input_by_ulps_and_by_no_more_than_the_count(upsampling_excess):
    e = upsampling_excess
    print("bilinear x2 up-sampling, worst excess over the largest input in units of 2^-24 of it: one axis %.3f; constant planes %.3f "
          "(H = %d, W = %d, value %.9g); alternating planes %.3f; counted n = %d" % ((e["one_axis"], e["constant"]) + e["at"] + (e["alternating"], AA.N_UP_AMAX)))
    assert e["one_axis"] > 0 and e["constant"] > 0, "the search found no excess: 'convex, x's bound holds' would be literally true"
    assert max(e["one_axis"], e["constant"], e["alternating"]) <= AA.N_UP_AMAX
    # the scale leaves room: a handed-on word exceeded by n 2^-24 keeps the largest fp16 operand below 2^15 (1 + 7 2^-24) < 65504
    assert 2.0 ** 15 * (1 + AA.N_UP_AMAX * U) < 65504.0


def test_mutant_upsampling_hand_on_without_the_counted_slack(monkeypatch, upsampling_excess):
    """The plane the search found, handed on with slack 0: the audit reports it; with the counted slack it is clean.  The audit knows
    the rule by the code object of hipnn's up-sampling entry, which cannot run without a device: a stand-in with the same call shape
    (x's word handed on to the up-sampled tensor) takes its place here, the up-sampled tensor comes from the twin."""
    H, W, M = upsampling_excess["at"]
    x = np.full((1, 1, H, W), M, dtype=np.float32)
    up = torch.from_numpy(R.upsample2x_twin32(x))
    assert float(up.max()) > M

    def upsample_bilinear2x_module(m, src):
        return HF.hand_on_amax(src, up.clone())
    monkeypatch.setattr(HF, "upsample_bilinear2x_module", upsample_bilinear2x_module)

    def build():
        return [HF.upsample_bilinear2x_module(None, _tagged(torch.from_numpy(x)))]
    a = _audited(monkeypatch, build)
    a.assert_clean()
    assert a.rules == {"hand_on:upsample": 1, "produced:_tagged": 1}      # (the source's own word is audited as it is handed on)
    a = _audited(monkeypatch, build, up_slack=0)
    assert len(a.violations) == 1, a.report()
