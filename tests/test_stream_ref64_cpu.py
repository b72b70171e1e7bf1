"""Pins tests/stream_ref64.py (the float64 references of the every-element checks of the streaming kernels) and proves that its bounds bite.

* torch's own CPU fp32 up-sampling and its gradient pass the derived bounds at every element; the two references are each other's
  transposes; a PURE float64 interpolation is more than 50 units of the bound away at W = 1030, which is why the coordinates are float32;
* a float32 twin of each kernel's expression passes (with the multiply-adds rounded separately and as fmas), and each mutant -- the kind
  of slip such a kernel makes -- fails at at least one element;
* the uint8 store rule at its stated edges; the warp oracle reproduces the reference module's goldens bit for bit.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import warp_numpy
from stream_ref64 import (N_ADAM_M, N_ADAM_P, N_ADAM_V, N_UP, N_UP_BWD, U, adam_inputs, adam_ref64, adam_scalars, assert_within_rounding,
                          axis_coords, f32_to_u8_ref, rounding_report, upsample2x_backward_ref64, upsample2x_ref64)

# (planes, H, W): the small shapes of test_stream_allelems_gpu.py, then [2,3,130,200] and [1,2,37,1030]
FWD_SHAPES = [(3, 5, 6), (2, 1, 2), (5, 7, 62), (3, 3, 64), (2, 33, 126), (3, 4, 128), (6, 130, 200), (2, 37, 1030)]
BWD_SHAPES = [(3, 5, 7), (2, 1, 1), (2, 9, 33), (2, 5, 65), (6, 130, 200), (2, 37, 1030)]
MUTANT_SHAPE = (2, 37, 1030)


def _planes(seed, P, H, W):
    return torch.randn(P, H, W, generator=torch.Generator().manual_seed(seed))


def _interp(x):
    return F.interpolate(x[None], scale_factor=2, mode="bilinear", align_corners=True)[0]


# ---- the references against torch's CPU kernels -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P,H,W", FWD_SHAPES)
def test_torch_cpu_fp32_upsampling_is_inside_the_forward_bound(P, H, W):
    x = _planes(100 + W, P, H, W)
    ref, S = upsample2x_ref64(x)
    assert ref.shape == (P, 2 * H, 2 * W) and ref.dtype == torch.float64 and (S >= ref.abs()).all()
    worst = assert_within_rounding(_interp(x), ref, S, N_UP, "torch CPU fp32 up-sampling %dx%dx%d" % (P, H, W))
    print("torch CPU fp32 up-sampling %dx%dx%d: worst err / (2^-24 S) = %.2f" % (P, H, W, worst))


@pytest.mark.parametrize("P,H,W", BWD_SHAPES)
def test_torch_cpu_fp32_upsampling_gradient_is_inside_the_backward_bound(P, H, W):
    g = _planes(200 + W, P, 2 * H, 2 * W)
    x = torch.zeros(P, H, W, requires_grad=True)
    _interp(x).backward(g)
    ref, S = upsample2x_backward_ref64(g, H, W)
    assert ref.shape == (P, H, W) and (S >= ref.abs()).all()
    worst = assert_within_rounding(x.grad, ref, S, N_UP_BWD, "torch CPU fp32 up-sampling gradient %dx%dx%d" % (P, H, W))
    print("torch CPU fp32 up-sampling gradient %dx%dx%d: worst err / (2^-24 S) = %.2f" % (P, H, W, worst))


@pytest.mark.parametrize("P,H,W", BWD_SHAPES)
def test_the_two_upsampling_references_are_transposes(P, H, W):
    """<up(x), g> = <x, up^T(g)>: the einsum of weight matrices and the gathers of the forward reference are two spellings of one map."""
    x, g = _planes(300 + W, P, H, W), _planes(301 + W, P, 2 * H, 2 * W)
    fwd, _ = upsample2x_ref64(x)
    bwd, _ = upsample2x_backward_ref64(g, H, W)
    a, b = float((fwd * g.double()).sum()), float((x.double() * bwd).sum())
    scale = float((fwd.abs() * g.double().abs()).sum())
    assert abs(a - b) <= 1e-13 * scale


def test_a_pure_float64_interpolation_is_far_outside_the_bound_at_w_1030():
    """The rounding of the float32 source coordinate moves the result by thousands of units: the references must take it in float32, and a
    criterion measured from a float64 interpolation (the project's older one) cannot be tight."""
    x = _planes(7, 2, 37, 1030)
    ref, S = upsample2x_ref64(x)
    rep = rounding_report(_interp(x.double()).float(), ref, S, 50)
    print("float64 F.interpolate against the float32-coordinate reference at W = 1030: %d elements beyond 50 units, worst %.0f"
          % (rep["bad"], rep["worst"]))
    assert rep["bad"] > 0 and rep["worst"] > 50


def test_the_last_position_of_every_axis_is_exactly_n_minus_1():
    """float32((n-1)/(2n-1)) * (2n-1) rounds back to n - 1 for every n the entry points take a plane of here: the last output reads
    source n - 1 with weight l1 = 0 on its clamped neighbour, so the clamp is a matter of memory safety and of 0 x Inf only."""
    for n in list(range(1, 2050)) + [4096, 8191, 16383, 16384]:
        i0, i1, l0, l1 = axis_coords(n)
        assert int(i0[-1]) == n - 1 and int(i1[-1]) == n - 1 and float(l1[-1]) == 0.0 and float(l0[-1]) == 1.0, n
        assert int(i1.max()) <= n - 1 and float(l1.min()) >= 0.0 and float(l1.max()) < 1.0


# ---- float32 twins of the up-sampling kernels and their mutants ----------------------------------------------------------------------------

def _coords_twin(n, mutant):
    """axis_coords as the kernels compute it, or one of the slips."""
    o = torch.arange(2 * n, dtype=torch.float32)
    r = torch.tensor(float(n - 1), dtype=torch.float32) / torch.tensor(float(2 * n - 1), dtype=torch.float32) if n > 0 else None
    if mutant == "half_scale":
        r = torch.tensor(float(n) / float(2 * n), dtype=torch.float32)            # n / (2n): align_corners = False's scale
    if mutant == "unrounded_coordinate":
        s64 = r.double() * o.double()                                              # the product never rounded to float32
        i0 = s64.to(torch.int64)
        l1 = (s64 - i0.double()).float()
    else:
        s = r * o
        i0 = s.to(torch.int64)
        l1 = s - i0.float()
    l0 = torch.tensor(1.0) - l1
    if mutant == "weights_exchanged":
        l0, l1 = l1, l0
    return i0, l0, l1


def _lerp2(w0, a, w1, b, fused):
    if fused:                                             # fma(w1, b, fmul(w0, a)): the product is exact in float64
        return (w1.double() * b.double() + (w0 * a).double()).float()
    return w0 * a + w1 * b


def _upsample_twin(x, mutant=None, fused=True):
    """The expression of the three forward kernels in float32, on planes [P,H,W].  An unclamped ``+1`` is modelled on the flat buffer:
    past a row's end it reads the next row's first element, past the last plane's end a zero."""
    P, H, W = x.shape
    y0, l0y, l1y = _coords_twin(H, mutant)
    x0, l0x, l1x = _coords_twin(W, mutant)
    if mutant == "step_not_clamped":
        flat = torch.cat([x.reshape(-1), torch.zeros(W + 2)])
        base = (torch.arange(P)[:, None, None] * H + y0[None, :, None]) * W + x0[None, None, :]
        a0, a1, b0, b1 = flat[base], flat[base + 1], flat[base + W], flat[base + W + 1]
    else:
        y1 = y0 + (y0 < H - 1).long()
        x1 = x0 + (x0 < W - 1).long()
        ra, rb = x[:, y0], x[:, y1]
        a0, a1, b0, b1 = ra[:, :, x0], ra[:, :, x1], rb[:, :, x0], rb[:, :, x1]
    l0y, l1y = l0y[:, None], l1y[:, None]
    return _lerp2(l0y, _lerp2(l0x, a0, l1x, a1, fused), l1y, _lerp2(l0x, b0, l1x, b1, fused), fused)


@pytest.mark.parametrize("fused", [True, False], ids=["fma", "separate"])
@pytest.mark.parametrize("P,H,W", FWD_SHAPES)
def test_upsampling_twin_passes_the_forward_bound(P, H, W, fused):
    x = _planes(400 + W, P, H, W)
    ref, S = upsample2x_ref64(x)
    worst = assert_within_rounding(_upsample_twin(x, fused=fused), ref, S, N_UP, "float32 twin %dx%dx%d" % (P, H, W))
    assert worst <= 4.000001                              # the derived first-order count itself
    if fused and W in (6, 200):
        assert torch.equal(_upsample_twin(x, fused=True), _upsample_twin(x, "step_not_clamped", fused=True))      # finite data: no trace


@pytest.mark.parametrize("mutant", ["unrounded_coordinate", "half_scale", "weights_exchanged"])
def test_upsampling_mutants_fail_the_forward_bound(mutant):
    x = _planes(500, *MUTANT_SHAPE)
    ref, S = upsample2x_ref64(x)
    with pytest.raises(AssertionError) as e:
        assert_within_rounding(_upsample_twin(x, mutant), ref, S, N_UP, mutant)
    print(str(e.value))
    rep = rounding_report(_upsample_twin(x, mutant), ref, S, N_UP)
    assert rep["bad"] >= 1 and rep["worst"] > 50


def test_upsampling_mutant_unclamped_step_shows_only_beside_a_non_finite_value():
    """The last output of a row reads its clamped neighbour with weight exactly 0 (the test above), so reading one element too far changes
    nothing on finite data; beside an Inf it makes 0 x Inf = NaN.  Plane 0 is finite and plane 1 starts with an Inf: the correct twin
    keeps plane 0 inside the bound; the mutant's last output row of plane 0 reads the Inf as its "next row" and, in the bottom-right
    corner, as its "next column", and is not finite there."""
    P, H, W = 2, 5, 6
    x = _planes(501, P, H, W)
    x[1, 0, 0] = float("inf")
    ref, S = upsample2x_ref64(x[:1])
    assert_within_rounding(_upsample_twin(x)[:1], ref, S, N_UP, "twin beside an Inf")
    got = _upsample_twin(x, "step_not_clamped")[:1]
    rep = rounding_report(got, ref, S, N_UP)
    assert rep["bad"] >= 1 and rep["nonfinite"] == rep["bad"] and not torch.isfinite(got[0, 2 * H - 1, 2 * W - 1])
    assert torch.isfinite(got[0, :2 * H - 1, :2 * W - 1]).all()              # only the last output row and column can see it


def _matrix_twin(n, mutant):
    """[2n, n] float32 weights of the gather: (i0 == i ? l0 : 0) + (i1 == i ? l1 : 0), one float32 sum where both hit."""
    i0, l0, l1 = _coords_twin(n, mutant)
    i1 = (i0 + 1) % n if mutant == "step_not_clamped" else i0 + (i0 < n - 1).long()
    M = torch.zeros(2 * n, n)
    rows = torch.arange(2 * n)
    M.index_put_((rows, i0), l0, accumulate=True)
    M.index_put_((rows, i1), l1, accumulate=True)
    return M


def _upsample_backward_twin(g, H, W, mutant=None):
    """sum_o wy[o] * (sum_w wx[w] * g[o, w]) in float32: the kernel's two nested sums (its six candidates per axis are the non-zero
    columns of these matrices and zeros add exactly)."""
    return torch.matmul(_matrix_twin(H, mutant).t(), torch.matmul(g, _matrix_twin(W, mutant)))


@pytest.mark.parametrize("P,H,W", BWD_SHAPES)
def test_upsampling_backward_twin_passes_the_backward_bound(P, H, W):
    g = _planes(600 + W, P, 2 * H, 2 * W)
    ref, S = upsample2x_backward_ref64(g, H, W)
    assert_within_rounding(_upsample_backward_twin(g, H, W), ref, S, N_UP_BWD, "float32 gradient twin %dx%dx%d" % (P, H, W))


@pytest.mark.parametrize("mutant", ["unrounded_coordinate", "half_scale", "weights_exchanged"])
def test_upsampling_mutants_fail_the_backward_bound(mutant):
    P, H, W = MUTANT_SHAPE
    g = _planes(601, P, 2 * H, 2 * W)
    ref, S = upsample2x_backward_ref64(g, H, W)
    rep = rounding_report(_upsample_backward_twin(g, H, W, mutant), ref, S, N_UP_BWD)
    assert rep["bad"] >= 1 and rep["worst"] > 50


# ---- Adam: twin and mutants ---------------------------------------------------------------------------------------------------------------

ADAM_N = 200000
ADAM_HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
ADAM_CONFIGS = [(step, wd) for step in (1, 2, 1000) for wd in (0.0, 1e-2)]


@pytest.fixture(scope="module")
def adam_state():
    return adam_inputs(ADAM_N, torch.Generator().manual_seed(77))


def _adam_twin(p, g, m, v, wd, step, mutant=None):
    """adam_step's expression in float32 tensor operations (each rounded on its own; gi as the kernel's fmaf), or one of the slips."""
    k = adam_scalars(step=step, wd=wd, **ADAM_HP)
    gi = g
    if k["wd"] != 0.0 and mutant != "decoupled_decay":
        gi = (k["wd"] * p.double() + g.double()).float()
    mi = m + (gi - m) * k["c1"]
    gv = g if mutant == "v_from_undecayed_gradient" else gi
    vi = k["b2"] * v + k["c2"] * gv * gv
    if mutant == "eps_inside_sqrt":
        denom = (vi + k["eps"]).sqrt() / k["bc2s"]
    elif mutant == "bc2_not_rooted":
        denom = vi.sqrt() / (k["bc2s"] * k["bc2s"]) + k["eps"]
    else:
        denom = vi.sqrt() / k["bc2s"] + k["eps"]
    base = p * (1.0 - k["lr"] * k["wd"]) if mutant == "decoupled_decay" else p
    return base - k["step_size"] * (mi / denom), mi, vi


def _adam_reports(state, wd, step, mutant=None):
    p, g, m, v = state
    p1, m1, v1, S_p, S_m, S_v = adam_ref64(p, g, m, v, wd=wd, step=step, **ADAM_HP)
    tp, tm, tv = _adam_twin(p, g, m, v, wd, step, mutant)
    return (rounding_report(tp, p1, S_p, N_ADAM_P), rounding_report(tm, m1, S_m, N_ADAM_M), rounding_report(tv, v1, S_v, N_ADAM_V))


def test_adam_inputs_reach_the_corners(adam_state):
    p, g, m, v = adam_state
    assert 0.005 * ADAM_N < int((g == 0).sum()) < 0.02 * ADAM_N and 0.005 * ADAM_N < int((v == 0).sum()) < 0.02 * ADAM_N
    assert float(g.abs()[g != 0].min()) < 1e-8 and float(g.abs().max()) > 10.0
    root = v.double().sqrt()
    assert int((root < 1e-9).sum()) > 1000 and int((root > 1e-7).sum()) > 1000          # eps = 1e-8 decides some, is noise for others
    assert (v >= 0).all()


@pytest.mark.parametrize("step,wd", ADAM_CONFIGS)
def test_adam_twin_passes_every_bound(adam_state, step, wd):
    reps = _adam_reports(adam_state, wd, step)
    print("Adam twin, step %d, wd %g: worst err / (2^-24 S) p %.3f, m %.2f, v %.2f" % (step, wd, reps[0]["worst"], reps[1]["worst"], reps[2]["worst"]))
    assert [r["bad"] for r in reps] == [0, 0, 0], reps


def test_adam_twin_agrees_with_torch_optim_adam(adam_state):
    """The reference is torch.optim.Adam's step, not only the kernel's: one step of the optimizer itself (float64) from the same state."""
    p, g, m, v = (t[:5000].double() for t in adam_state)
    k = adam_scalars(step=3, wd=1e-2, **ADAM_HP)
    w = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([w], lr=k["lr"], betas=(k["b1"], k["b2"]), eps=k["eps"], weight_decay=k["wd"])
    opt.state[w] = {"step": torch.tensor(2.0), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    w.grad = g.clone()
    opt.step()
    p1, m1, v1, S_p, S_m, S_v = adam_ref64(*(t[:5000] for t in adam_state), wd=1e-2, step=3, **ADAM_HP)
    # the reference rounds bc1, sqrt(bc2), 1 - beta and lr / bc1 to float32 as the kernel does: within a few 2^-24 of the optimizer
    assert ((w.detach() - p1).abs() <= 4 * U * S_p).all()
    assert ((opt.state[w]["exp_avg"] - m1).abs() <= 2 * U * S_m).all() and ((opt.state[w]["exp_avg_sq"] - v1).abs() <= 2 * U * S_v).all()


@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("mutant,wds", [("eps_inside_sqrt", (0.0, 1e-2)), ("bc2_not_rooted", (0.0, 1e-2)),
                                        ("decoupled_decay", (1e-2,)), ("v_from_undecayed_gradient", (1e-2,))])
def test_adam_mutants_fail(adam_state, mutant, wds, step):
    for wd in wds:
        reps = _adam_reports(adam_state, wd, step, mutant)
        print("Adam mutant %s, step %d, wd %g: elements outside the bound p %d, m %d, v %d" % (mutant, step, wd, *(r["bad"] for r in reps)))
        assert reps[0]["bad"] >= 1 or reps[2]["bad"] >= 1, (mutant, step, wd)
        assert reps[0]["bad"] >= 1                       # every one of these slips reaches the parameter
    if mutant in ("decoupled_decay", "v_from_undecayed_gradient"):
        assert [r["bad"] for r in _adam_reports(adam_state, 0.0, step, mutant)] == [0, 0, 0]      # without decay they are the same step


# ---- the uint8 store rule -----------------------------------------------------------------------------------------------------------------

def test_u8_rule_at_its_edges():
    f = np.float32
    n256, m1 = f(256.0) / f(255.0), f(-1.0) / f(255.0)
    vals = [0.0, -0.0, 0.5, 1.0, 2.0, -1.0, -0.999, n256, np.nextafter(n256, f(0)), np.nextafter(n256, f(2)),
            m1, np.nextafter(m1, f(0)), np.nextafter(m1, f(-1)), 1e10, -1e10, 4e16, 1e19, -1e19, np.inf, -np.inf, np.nan, 3.5e16, -3.5e16]
    v = torch.tensor(np.array(vals, f))
    t = (v.numpy() * f(255.0)).astype(np.float64)                            # the rounded float32 products, as exact numbers
    want = [0 if (not np.isfinite(x) or abs(x) >= 9e18) else int(x) % 256 for x in t]          # int() truncates; % 256 keeps the low 8 bits
    assert f32_to_u8_ref(v, 0).tolist() == want
    at = lambda x: want[vals.index(x)]
    assert at(-1.0) == 1 and want[1] == 0 and at(2.0) == 254 and at(1.0) == 255 and at(0.5) == 127
    assert abs(t[vals.index(4e16)]) >= 9e18 > abs(t[vals.index(3.5e16)]) and at(4e16) == 0           # on either side of 9e18
    # scaled values 256.0 -> 0 and -1.0 -> 255, as the kernel's comment states them
    scaled = {float(x): u for x, u in zip(t, want)}
    assert scaled[256.0] == 0 and scaled[-1.0] == 255
    clamped = f32_to_u8_ref(v, 1).tolist()
    for x, u in zip(vals, clamped):
        assert u == (0 if (np.isnan(x) or x < 0) else 255 if x > 1 else int(f(x) * f(255.0))), x
    # inside [0, 256) the rule is numpy's astype
    r = torch.rand(4096, generator=torch.Generator().manual_seed(3)) * 1.5 - 0.2
    r = r[(r * 255 > -1) & (r * 255 < 256)]
    assert np.array_equal(f32_to_u8_ref(r, 0).numpy(), (r.numpy() * f(255.0)).astype(np.int64).astype(np.uint8))


# ---- the warp oracle ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["small", "edge", "c1"])
def test_warp_oracle_reproduces_the_reference_goldens_bit_for_bit(golden_dir, name):
    gold = np.load(os.path.join(golden_dir, "warp.npz"))
    assert np.array_equal(warp_numpy.warp(gold[name + "_img"], gold[name + "_flow"]), gold[name + "_out"])
