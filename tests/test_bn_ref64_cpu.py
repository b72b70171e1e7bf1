"""Pins tests/bn_ref64.py (the float64 reference and the derived bounds of the every-element BatchNorm checks) and proves that the bounds
bite, without a GPU.

* bn_ref64 equals torch's own float64 nn.BatchNorm2d + activation under autograd: output, running statistics, all three gradients;
* bn_geometry against the hand-computed table of the shapes test_bn_allelems_gpu.py runs;
* a numpy float32 twin of csrc/norm_kernels.hip -- chunks, pivot, the per-thread order of both load paths, the double tree, the float32
  triplets, Chan's merge in double, multiply-adds as one rounding (and, to show that the counts hold either way, as two) -- passes
  every bound at the small shapes, on the conditioning channels and on hand-made partials;
* each mutant of the twin -- the kind of slip such a kernel makes -- fails;
* the mask fixture has teeth: with the activation mask recomputed as (x - mean) * invstd * w + b, the backward this kernel had, the twin
  disagrees with its own forward at every element holding the targeted grid value in at least two channels, and misses the dx and
  dbias bounds there; with the forward's own expression it passes.
"""
import numpy as np
import pytest
import torch

import bn_ref64 as R
from bn_ref64 import ACT_LEAKY, ACT_NONE, ACT_RELU, ACTS, CONFIGS, EPS, SHAPES, SMALL
from stream_ref64 import rounding_report

F = np.float32
D = np.float64
TH = R.BN_THREADS


# ---- the reference against torch's float64 modules ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("act,slope", ACTS)
@pytest.mark.parametrize("shape", [(2, 3, 35), (2, 4, 1), (3, 5, 3079), (300, 2, 6)])
def test_reference_equals_torch_float64_autograd(shape, act, slope):
    N, C, HW = shape
    g = torch.Generator().manual_seed(5 + HW)
    inp = R.case_inputs(shape, CONFIGS[0], g)
    eps, mom, sl = R.f32(EPS), R.f32(0.1), R.f32(slope)
    bn = torch.nn.BatchNorm2d(C, eps=eps, momentum=mom).double().train()
    with torch.no_grad():
        bn.weight.copy_(inp["weight"]); bn.bias.copy_(inp["bias"])
        bn.running_mean.copy_(inp["running_mean"]); bn.running_var.copy_(inp["running_var"])
    xr = inp["x"].double().view(N, C, HW, 1).requires_grad_()
    pre = bn(xr)
    assert float(pre.detach().abs().min()) > 1e-6                 # no pre-activation near zero: torch's mask and any other agree
    yr = {ACT_NONE: lambda t: t, ACT_RELU: torch.relu, ACT_LEAKY: lambda t: torch.nn.functional.leaky_relu(t, sl)}[act](pre)
    yr.backward(inp["dy"].double().view(N, C, HW, 1))
    st = R.bn_stats_ref64(inp["x"], EPS, 0.1, inp["running_mean"], inp["running_var"], R.kernel_chunks(inp["x"]))
    y, S_y = R.bn_apply_ref64(inp["x"], st["mean"], st["invstd"], inp["weight"], inp["bias"], act, slope)
    bw = R.bn_backward_ref64(inp["dy"], inp["x"], y, st["mean"], st["invstd"], inp["weight"], act, slope, 4)
    # 1e-12 of the magnitude of the terms each result sums (with two values per channel dx itself is a complete cancellation)
    close = lambda a, b, S: bool(((a - b).abs() <= 1e-12 * S).all())
    assert close(y, yr.detach().view(N, C, HW), S_y)
    assert close(st["running_mean"], bn.running_mean, bn.running_mean.abs()) and close(st["running_var"], bn.running_var, bn.running_var.abs())
    assert close(bw["dx"], xr.grad.view(N, C, HW), bw["S_dx"])
    assert close(bw["dweight"], bn.weight.grad, bw["S_dweight"]) and close(bw["dbias"], bn.bias.grad, bw["S_dbias"])


def test_geometry_table():
    for shape, geometry in SHAPES:
        assert R.bn_geometry(*shape) == geometry, shape
    assert R.bn_geometry(*R.MASK_SHAPE) == (1024, 2, 4)
    assert R.bn_geometry(2, 3, 1100) == (1024, 2, 4)
    assert R.bn_geometry(16, 32, 65536) == (16384, 4, 64) and R.bn_geometry(2, 64, 16384) == (2048, 8, 16)
    assert max(N * C * HW for (N, C, HW), _ in SHAPES) == 512 * 16389 < 8.4e6


# ---- the float32 twin ---------------------------------------------------------------------------------------------------------------------

def _fma(a, b, c, fused):
    """a * b + c in float32: one rounding (taken from the float64 value of the exact product plus c) or two."""
    if fused:
        return (np.asarray(a, D) * np.asarray(b, D) + np.asarray(c, D)).astype(F)
    return (np.asarray(a, F) * np.asarray(b, F)).astype(F) + np.asarray(c, F)


def _tree(v):
    """block_sum2: the fixed tree over the 256 per-thread doubles."""
    v = np.array(v, D)
    o = TH // 2
    while o:
        v[..., :o] += v[..., o:2 * o]
        o >>= 1
    return v[..., 0]


def _strided(vals):
    """[C, P] doubles -> [C]: thread t sums entries t, t + 256, ... in order, then the tree (channel_moments / channel_totals)."""
    C, P = vals.shape
    rounds = -(-P // TH)
    pad = np.zeros((C, rounds * TH), D)
    pad[:, :P] = vals
    acc = np.zeros((C, TH), D)
    for r in range(rounds):
        acc += pad[:, r * TH:(r + 1) * TH]
    return _tree(acc)


class _Chunks:
    """The (channel, chunk) workgroups of a launch on [N, C, HW], channel-major, and their elements gathered into rows of a common
    padded length (a multiple of 1024); ``valid`` marks the real ones."""

    def __init__(self, N, C, HW):
        self.chunk_len, self.pieces, self.chunks = R.bn_geometry(N, C, HW)
        self.C, self.K = C, C * self.chunks
        self.Lpad = -(-min(self.chunk_len, HW) // 1024) * 1024
        c = np.repeat(np.arange(C), self.chunks)
        k = np.tile(np.arange(self.chunks), C)
        start = (k % self.pieces) * self.chunk_len
        self.len = np.minimum(HW - start, self.chunk_len)
        self.base = ((k // self.pieces) * C + c) * HW + start
        j = np.arange(self.Lpad)[None, :]
        self.valid = j < self.len[:, None]
        self.idx = np.where(self.valid, self.base[:, None] + j, 0)
        self.aligned = (self.base % 4) == 0

    def gather(self, t):
        return np.where(self.valid, t.reshape(-1)[self.idx], F(0))

    def thread_sums(self, a, b, fused, drop_tail=False):
        """Per workgroup and thread, in the kernels' order: s += a and q = b * a' + q over the thread's elements, a' = a where b is None
        (forward: a = x - pivot) or the second operand (backward: a = dz, b = xhat).  Both load paths, chosen per workgroup by the
        alignment of its base.  Padding is zero and adds exactly."""
        K, Lp = a.shape
        b = a if b is None else b
        s1, q1 = np.zeros((K, TH), F), np.zeros((K, TH), F)                    # scalar path: element i -> thread i % 256
        for r in range(Lp // TH):
            av, bv = a[:, r * TH:(r + 1) * TH], b[:, r * TH:(r + 1) * TH]
            s1 = s1 + av
            q1 = _fma(av, bv, q1, fused)
        ng = self.len // 4                                                      # vector path: group g of four -> thread g % 256
        NG = Lp // 4
        gm = (np.arange(NG)[None, :] < ng[:, None])[:, :, None]
        ag, bg = np.where(gm, a.reshape(K, NG, 4), F(0)), np.where(gm, b.reshape(K, NG, 4), F(0))
        s4, q4 = np.zeros((K, TH), F), np.zeros((K, TH), F)
        for r in range(NG // TH):
            av, bv = ag[:, r * TH:(r + 1) * TH], bg[:, r * TH:(r + 1) * TH]
            if b is a:                                                          # (v.x + v.y) + (v.z + v.w); (x^2 + y^2) + (z^2 + w^2)
                s4 = s4 + ((av[..., 0] + av[..., 1]) + (av[..., 2] + av[..., 3]))
                q4 = q4 + (_fma(av[..., 0], av[..., 0], av[..., 1] * av[..., 1], fused) + _fma(av[..., 2], av[..., 2], av[..., 3] * av[..., 3], fused))
            else:                                                               # one(x), one(y), one(z), one(w) in turn
                for lane in range(4):
                    s4 = s4 + av[..., lane]
                    q4 = _fma(av[..., lane], bv[..., lane], q4, fused)
        if not drop_tail:
            rows = np.arange(K)
            for t in range(3):
                i = 4 * ng + t
                ok = i < self.len
                av = np.where(ok, a[rows, np.minimum(i, Lp - 1)], F(0))
                bv = np.where(ok, b[rows, np.minimum(i, Lp - 1)], F(0))
                s4[:, t] = s4[:, t] + av
                q4[:, t] = _fma(av, bv, q4[:, t], fused)
        al = self.aligned[:, None]
        return np.where(al, s4, s1), np.where(al, q4, q1)


def _act(pre, act, slope, mutant=None):
    if act == ACT_RELU:
        return np.where(pre > 0, pre, F(0))
    if act == ACT_LEAKY:
        if mutant == "slope_on_the_positive_side":
            return np.where(pre > 0, pre * F(slope), pre)
        return np.where(pre > 0, pre, pre * F(slope))
    return pre


def twin_forward(x, weight, bias, rm, rv, momentum, eps, act, slope, fused=True, mutant=None, partials=None):
    """bn_fwd_partial + bn_fwd_apply (or the apply alone on given float32 ``partials`` [C, P, 3]) on x [N, C, HW] float32."""
    N, C, HW = x.shape
    ch = _Chunks(N, C, HW)
    if partials is None:
        P = ch.gather(x)
        pivot = P[:, :1]
        V = np.where(ch.valid, P - pivot, F(0))
        s, q = ch.thread_sums(V, None, fused, drop_tail=(mutant == "tail_dropped"))
        ds, dq = _tree(s), _tree(q)
        n = ch.len.astype(D)
        dm = ds / n
        part = np.stack([ch.len.astype(F), (pivot[:, 0].astype(D) + dm).astype(F), np.maximum(dq - ds * dm, 0.0).astype(F)], 1)
        part = part.reshape(C, ch.chunks, 3)
    else:
        part = partials
    t = part.astype(D)
    cnt_w = np.where(t[..., 0] > 0, t[..., 0], 1.0) if mutant == "empty_partials_count" else t[..., 0]
    cnt = _strided(t[..., 0])
    mean = _strided(cnt_w * t[..., 1]) / cnt
    d = t[..., 1] - mean[:, None]
    var = _strided(t[..., 2] + cnt_w * d * d) / cnt
    if mutant == "fp32_square_minus_mean_square":                  # E[x^2] - E[x]^2 in float32
        xc = x.transpose(1, 0, 2).reshape(C, -1)
        m32 = (np.sum(xc, axis=1, dtype=F) / F(N * HW)).astype(F)
        var = np.maximum((np.sum(xc * xc, axis=1, dtype=F) / F(N * HW)).astype(F) - m32 * m32, F(0)).astype(D)
        mean = m32.astype(D)
    mean32 = mean.astype(F)
    invstd = (1.0 / np.sqrt(var + D(F(eps)))).astype(F)
    out = {"save_mean": mean32, "save_invstd": invstd, "running_mean": None, "running_var": None, "part": part}
    mom = F(momentum)
    c1 = F(1) - mom
    if rm is not None:
        out["running_mean"] = _fma(c1, rm, mom * mean32, fused)
    if rv is not None:
        unbiased = np.where(cnt > 1, var * cnt / np.maximum(cnt - 1.0, 1.0), var)
        if mutant == "biased_running_var":
            unbiased = var
        out["running_var"] = _fma(c1, rv, mom * unbiased.astype(F), fused)
    w = np.ones(C, F) if weight is None else weight
    b = np.zeros(C, F) if bias is None else bias
    sc = invstd * w
    sf = _fma(-mean32, sc, b, fused)
    pre = _fma(x, sc[None, :, None], sf[None, :, None], fused)
    out["pre"] = pre
    out["y"] = _act(pre, act, slope, mutant)
    return out


def twin_backward(dy, x, weight, bias, mean, invstd, act, slope, fused=True, mask="forward", mutant=None, prior_dw=None, prior_db=None,
                  want_pgrads=True):
    """bn_bwd_partial + bn_bwd_apply.  ``mask``: "forward" takes act' at the forward's own fma(x, sc, sf); "xhat" at
    fma((x - mean) * invstd, w, b), the expression the backward had before it was matched to the forward."""
    N, C, HW = x.shape
    ch = _Chunks(N, C, HW)
    w = np.ones(C, F) if weight is None else weight
    b = np.zeros(C, F) if bias is None else bias
    col = lambda v: v[None, :, None]
    xh = ((x - col(mean)).astype(F) * col(invstd)).astype(F)
    if mask == "forward":
        sc = invstd * w
        pre = _fma(x, col(sc), col(_fma(-mean, sc, b, fused)), fused)
    else:
        pre = _fma(xh, col(w), col(b), fused)
    grad = {ACT_NONE: F(1), ACT_RELU: np.where(pre > 0, F(1), F(0)), ACT_LEAKY: np.where(pre > 0, F(1), F(slope))}[act]
    dz = (dy * grad).astype(F)
    s, q = ch.thread_sums(ch.gather(dz), ch.gather(xh), fused)
    part = np.stack([_tree(s).astype(F), _tree(q).astype(F)], 1).reshape(C, ch.chunks, 2).astype(D)
    sdz, sdzx = _strided(part[..., 0]), _strided(part[..., 1])
    out = {"dweight": None, "dbias": None}
    if want_pgrads:
        out["dbias"], out["dweight"] = sdz.astype(F), sdzx.astype(F)
        if prior_db is not None and mutant != "accumulate_ignores_the_prior":
            out["dbias"], out["dweight"] = prior_db + out["dbias"], prior_dw + out["dweight"]
    cnt = D(HW) if mutant == "means_over_hw" else D(N) * D(HW)
    m_dz, m_dzx = (sdz / cnt).astype(F), (sdzx / cnt).astype(F)
    k = w * invstd
    inner = _fma(-xh, col(m_dzx), dz - col(m_dz), fused)
    out["dx"] = (col(k) * inner).astype(F)
    out["pre"] = pre
    return out


def _np(t):
    return None if t is None else t.numpy()


def _th(d, keys):
    return {k: (None if d.get(k) is None else torch.from_numpy(np.ascontiguousarray(d[k]))) for k in keys}


def _run_twin(inp, cfg, act, slope, fused=True, mutant=None, partials=None, table=None, mask="forward", what="twin"):
    """Forward and backward twins on a case, every bound asserted; returns (forward outputs, backward outputs, worst ratios)."""
    x = inp["x"].numpy()
    N, C, HW = x.shape
    fw = twin_forward(x, _np(inp["weight"]), _np(inp["bias"]), _np(inp["running_mean"]), _np(inp["running_var"]), cfg["momentum"], EPS,
                      act, slope, fused, mutant, partials)
    T = R.threads_terms(R.bn_geometry(N, C, HW)[0])
    bw = twin_backward(inp["dy"].numpy(), x, _np(inp["weight"]), _np(inp["bias"]), fw["save_mean"], fw["save_invstd"], act, slope, fused, mask,
                       mutant, _np(inp["prior_dweight"]), _np(inp["prior_dbias"]), cfg["pgrads"])
    got_f = _th(fw, ("y", "save_mean", "save_invstd", "running_mean", "running_var"))
    got_b = _th(bw, ("dx", "dweight", "dbias"))
    table = R.kernel_chunks(inp["x"]) if table is None else table
    worst = R.check_forward(got_f, inp, cfg["momentum"], EPS, act, slope, table, what)
    worst.update(R.check_backward(got_b, inp, got_f["y"], got_f["save_mean"], got_f["save_invstd"], act, slope, T, what))
    return fw, bw, worst


def _case(i, seed=0):
    shape, _ = SHAPES[i]
    return R.case_inputs(shape, CONFIGS[i], torch.Generator().manual_seed(100 + i + seed))


@pytest.mark.parametrize("fused", [True, False], ids=["fma", "separate"])
@pytest.mark.parametrize("act,slope", ACTS)
@pytest.mark.parametrize("i", range(SMALL))
def test_twin_passes_every_bound(i, act, slope, fused):
    _, _, worst = _run_twin(_case(i), CONFIGS[i], act, slope, fused, what="twin %s" % (SHAPES[i][0],))
    print("twin %s act %d: worst err / bound %s" % (SHAPES[i][0], act, {k: round(v, 3) for k, v in worst.items()}))
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("fused", [True, False], ids=["fma", "separate"])
def test_twin_passes_on_the_conditioning_channels(fused):
    inp = R.conditioning_inputs(torch.Generator().manual_seed(31))
    fw, _, worst = _run_twin(inp, CONFIGS[0], ACT_LEAKY, 0.2, fused, what="twin, conditioning")
    print("twin, conditioning: worst err / bound %s" % {k: round(v, 3) for k, v in worst.items()})
    st = R.bn_stats_ref64(inp["x"], EPS, 0.1, None, None, R.kernel_chunks(inp["x"]))
    assert float(st["S_invstd"][0]) < 400.0                          # the large-mean channel is held to some hundreds of u, not to u * mean^2
    assert fw["save_mean"][1] == F(-3.25) and fw["save_invstd"][1] == F(1.0 / np.sqrt(D(F(EPS))))          # variance exactly 0
    assert (fw["part"][1, :, 2] == 0).all()


@pytest.mark.parametrize("n_partials", [1, 7, 300])
@pytest.mark.parametrize("i", [0, 1, 3])
def test_twin_passes_on_hand_made_partials(i, n_partials):
    inp = _case(i, seed=50)
    trip, table = R.partition_triplets(inp["x"], n_partials, seed=7 * n_partials + i)
    assert n_partials < 7 or bool((trip[..., 0] == 0).any())          # some runs are empty
    _run_twin(inp, CONFIGS[i], ACT_RELU, 0.0, partials=trip.numpy(), table=table, what="twin, %d partials" % n_partials)


# ---- mutants ------------------------------------------------------------------------------------------------------------------------------

def _fails(**kw):
    with pytest.raises(AssertionError) as e:
        _run_twin(**kw)
    print(str(e.value)[:300])
    return str(e.value)


def test_mutant_biased_variance_into_running_var():
    assert "running_var" in _fails(inp=_case(0), cfg=CONFIGS[0], act=ACT_NONE, slope=0.0, mutant="biased_running_var")


def test_mutant_fp32_square_minus_mean_square_on_the_large_mean_channel():
    inp = R.conditioning_inputs(torch.Generator().manual_seed(31))
    assert "save_invstd" in _fails(inp=inp, cfg=dict(CONFIGS[0], running=False), act=ACT_NONE, slope=0.0, mutant="fp32_square_minus_mean_square")
    inp["x"][:, 0] -= 1000.0                                           # without the large mean the same slip is inside the bound's reach
    inp["running_mean"] = inp["running_var"] = None
    x = inp["x"].numpy()
    fw = twin_forward(x, None, None, None, None, 0.1, EPS, ACT_NONE, 0.0, mutant="fp32_square_minus_mean_square")
    ok = twin_forward(x, None, None, None, None, 0.1, EPS, ACT_NONE, 0.0)
    assert abs(float(fw["save_invstd"][0]) - float(ok["save_invstd"][0])) < 1e-5 * float(ok["save_invstd"][0])


def test_mutant_tail_elements_dropped():
    msg = _fails(inp=_case(3), cfg=CONFIGS[3], act=ACT_NONE, slope=0.0, mutant="tail_dropped")
    assert "save_mean" in msg or "save_invstd" in msg
    # the last chunk of (1, 2, 1025) is one element, its own pivot: x - pivot = 0 adds nothing, so dropping it leaves no trace THERE
    _run_twin(_case(2), CONFIGS[2], ACT_NONE, 0.0, mutant="tail_dropped")


def test_mutant_means_divided_by_hw():
    assert ": dx" in _fails(inp=_case(0), cfg=CONFIGS[0], act=ACT_RELU, slope=0.0, mutant="means_over_hw")


def test_mutant_accumulate_ignores_the_prior():
    assert CONFIGS[2]["accumulate"] == 1
    msg = _fails(inp=_case(2), cfg=CONFIGS[2], act=ACT_RELU, slope=0.0, mutant="accumulate_ignores_the_prior")
    assert "dweight" in msg or "dbias" in msg


def test_mutant_slope_on_the_positive_side():
    assert ": y" in _fails(inp=_case(0), cfg=CONFIGS[0], act=ACT_LEAKY, slope=0.2, mutant="slope_on_the_positive_side")


def test_mutant_empty_partials_contribute_their_mean():
    inp = _case(0, seed=50)
    trip, table = R.partition_triplets(inp["x"], 300, seed=3)
    assert int((trip[..., 0] == 0).sum()) > 100
    msg = _fails(inp=inp, cfg=CONFIGS[0], act=ACT_NONE, slope=0.0, mutant="empty_partials_count", partials=trip.numpy(), table=table)
    assert "save_mean" in msg


# ---- the mask fixture ---------------------------------------------------------------------------------------------------------------------

def _mask_case(fused=True):
    x, weight, dy, target = R.mask_fixture()
    first = twin_forward(x.numpy(), weight.numpy(), np.zeros(8, F), None, None, 0.1, EPS, ACT_NONE, 0.0, fused)
    bias = R.mask_bias(torch.from_numpy(first["save_mean"]), torch.from_numpy(first["save_invstd"]), weight, target)
    inp = {"x": x, "dy": dy, "weight": weight, "bias": bias, "running_mean": None, "running_var": None, "prior_dweight": None, "prior_dbias": None}
    return inp, target


@pytest.mark.parametrize("act,slope", ACTS[1:])
def test_mask_fixture_has_teeth_under_the_old_backward_expression(act, slope):
    """The condition on the fixture: in the float32 emulation the OLD mask expression disagrees with the forward in at least one channel
    (here: at least two), at every element holding the targeted value and nowhere else; that twin fails the dx bound by orders of
    magnitude and dbias by a whole dy, and the twin that shares the forward's expression passes everything."""
    inp, target = _mask_case()
    cfg = dict(CONFIGS[0], running=False)
    fw, bw, worst = _run_twin(inp, cfg, act, slope, what="mask fixture, forward's expression")
    assert np.array_equal(bw["pre"], fw["pre"])
    x = inp["x"].numpy()
    old = twin_backward(inp["dy"].numpy(), x, inp["weight"].numpy(), inp["bias"].numpy(), fw["save_mean"], fw["save_invstd"], act, slope, mask="xhat")
    differ = (old["pre"] > 0) != (fw["pre"] > 0)
    at_target = x == target.numpy()[None, :, None]
    assert not (differ & ~at_target).any()
    channels = [c for c in range(8) if differ[:, c].any()]
    for c in channels:
        assert (differ[:, c] == at_target[:, c]).all()                # every element holding the value, at once
    counts = [int(differ[:, c].sum()) for c in channels]
    print("old mask expression: channels %s disagree at %s elements of 4096" % (channels, counts))
    assert len(channels) >= 2 and min(counts) >= 3
    ref = R.bn_backward_ref64(inp["dy"], inp["x"], torch.from_numpy(fw["y"]), torch.from_numpy(fw["save_mean"]), torch.from_numpy(fw["save_invstd"]),
                              inp["weight"], act, slope, 4)
    rep = rounding_report(torch.from_numpy(old["dx"]), ref["dx"], ref["S_dx"], R.N_DX)
    assert rep["bad"] >= sum(counts) and rep["worst"] > 1e3 * R.N_DX
    assert rounding_report(torch.from_numpy(old["dbias"]), ref["dbias"], ref["S_dbias"], ref["n_dbias"])["bad"] >= 1
    with pytest.raises(AssertionError):
        _run_twin(inp, cfg, act, slope, mask="xhat")
