"""Float64 references of the streaming kernels for every-element checks (test infrastructure only; torch, any device).

The kernels of csrc/misc_kernels.hip run between the convolutions and the sepconv apply in every forward pass and training step:
bilinear x2 up-sampling and its gradient, the flat Adam update, the uint8 edge.  Each function below restates one of them as plain
tensor code that shares nothing with the kernels and runs on whatever device its inputs are on, so a kernel can be held at EVERY
element of the shapes where its launcher switches code paths.

    upsample2x_ref64(x)                                   -> (ref, S)     nn.Upsample(2, 'bilinear', align_corners=True) on [..., H, W]
    upsample2x_backward_ref64(g, H, W)                    -> (ref, S)     its exact transpose on [P, 2H, 2W]
    adam_ref64(p, g, m, v, lr, b1, b2, eps, wd, step)     -> (p', m', v', S_p, S_m, S_v)     one step of sstem_adam_step_f32
    f32_to_u8_ref(v, clamp01)                             -> uint8        the store rule of sstem_f32_to_gray_u8

What is taken in float32, and why
---------------------------------
The contract of the up-sampling kernels (and of torch's) fixes the source COORDINATE in float32:

    r = float32(n - 1) / float32(2n - 1)      one IEEE division          s  = r * float32(o)      one rounded product
    i0 = int(s)     l1 = s - i0 (exact)       l0 = float32(1) - l1       i1 = i0 + (i0 < n - 1)

A pure float64 interpolation differs from that by the rounding of ``s``, which moves the weights by up to ulp(n) / 2: 2e-4 of the data
at n = 1030, thousands of units of the bound below.  So the references take exactly these float32 numbers (``axis_coords``) and do
everything after them in float64.  Adam's scalars are float32 too: the entry point receives lr, beta1, beta2, eps, weight_decay as
floats, forms bc1 = 1 - beta1^step and sqrt(1 - beta2^step) in double and rounds them to float, and the kernel forms
1.f - beta1, 1.f - beta2 and lr / bc1 in float32 (``adam_scalars``; every one of these is a single correctly rounded operation on
float32 values, which float64 arithmetic followed by one rounding to float32 reproduces: 53 >= 2 * 24 + 2).

The acceptance bound
--------------------
As in sepconv_ref64: ``S`` is the sum of the magnitudes of the very terms the result sums, and an fp32 evaluation that spends m rounded
operations on the path of any one term errs by at most gamma_m * S, gamma_m = m u / (1 - m u), u = 2^-24 (Higham 3.1, 3.4), in any
order, fused or not.  ``assert_within_rounding`` checks  |got - ref| <= n * 2^-24 * S + 2^-120  at every element (2^-120: up to 64
operations whose result underflows lose at most 2^-126 each even where subnormals are flushed).  Every n is m counted from the kernel's
expression, rounded up to the next integer for gamma_m / (m u) - 1 < 1e-6 and the reference's own float64 error (below 2^-26 units);
none is tuned.  A multiply-add that the compiler contracts into one fma drops a rounding from a path and never adds one, so each count
is taken for the uncontracted form and holds for both.

* Up-sampling forward.  The weights are the same float32 numbers in the kernel and in the reference, so only the arithmetic on the
  values rounds.  lerp2(w0, a, w1, b) = fma(w1, b, fmul(w0, a)): the term w0 a passes the product and the sum (2), w1 b the sum (1).
  The horizontal lerp2 feeds the vertical one: at most 2 + 2 = 4 on the path of l0y l0x a0.  Uncontracted ((w0 a) + (w1 b), torch's CPU
  kernel) every term passes a product and a sum per axis: 4 again.  **N_UP = 5.**
* Up-sampling backward (a gather of 6 x 6 candidates per input pixel).  The kernel's weight of a candidate is (x0 == x ? l0 : 0) +
  (x1 == x ? l1 : 0): exact unless both hit, on the clamped last row / column, where l0 + l1 rounds once per axis (2; the reference
  adds the two in float64).  ``s += wx[j] * row[j]`` over six terms from s = 0: a product and at most five further sums (0 + x is
  exact) = 6; ``acc += wy[i] * s`` likewise 6.  2 + 6 + 6 = 14.  **N_UP_BWD = 15.**  (Three of the six weights per axis are zero and
  adding zero is exact, so a real launch stays far below; torch's own scatter-add stays within 4.)
* Adam.  With c1 = 1.f - beta1, c2 = 1.f - beta2, A = |g| + |wd p| (the magnitudes gi = fma(wd, p, g) sums; gi = g exactly at wd = 0):
    m' = m + (gi - m) c1        gi (1), the difference (1), the product (1), the sum (1): 4 on S_m = |m| + c1 (A + |m|).  **N_ADAM_M = 5.**
    v' = beta2 v + c2 gi gi     gi's rounding enters twice (2), the products c2 gi and (c2 gi) gi (2), the sum (1): 5 on
                                S_v = beta2 |v| + c2 A^2; the term beta2 v passes 2.  **N_ADAM_V = 6.**
    p' = p - step_size (m' / denom),  denom = sqrt(v') / sqrt(bc2) + eps.  sqrtf and the division are correctly rounded under hipcc's
    default (-fhip-fp32-correctly-rounded-divide-sqrt), one rounding each.  S_p is the sum of four terms, each with the count of the
    roundings that reach p' through it:
      1    |p'|                                        the final subtraction
      6.5  T1 = step_size |m' / denom|                 relative error of denom: v' from its own products and sum 3, halved by the root 1.5,
                                                       the root 1, the division by sqrt(bc2) 1, the sum with eps 1 = 4.5 (both terms of
                                                       denom are positive); then the quotient 1 and the product with step_size 1
      4    T2 = step_size S_m / denom                  the kernel divides ITS m', which carries N_ADAM_M's four roundings on S_m
                                                       (S_m <= (2 - beta1) (|m| + |g| + |wd p|))
      1    T3 = T1 sqrt(c2) A / (sqrt(bc2) denom)      gi's one rounding (at most u A, however far g and wd p cancel) reaches denom through
                                                       the root: |d sqrt(beta2 v + c2 x^2) / dx| <= sqrt(c2).  Zero at wd = 0.
    S_p = |p'| + 6.5 T1 + 4 T2 + T3, checked with **N_ADAM_P = 1.01** (the second-order products of these terms are below 1e-5 of them).
    T3 is what a count on T1 and T2 alone would miss: it matters only where g cancels against wd p AND v is near zero.
"""
import math

import torch

U = 2.0 ** -24
ABS_SLACK = 2.0 ** -120
N_UP = 5
N_UP_BWD = 15
N_ADAM_M = 5
N_ADAM_V = 6
N_ADAM_P = 1.01
ADAM_P_COUNTS = (1.0, 6.5, 4.0, 1.0)          # |p'|, T1, T2, T3


# ---- bilinear x2 up-sampling, align_corners = True --------------------------------------------------------------------------------------

def axis_coords(n, device="cpu"):
    """The 2n output positions of an axis of n source pixels: (i0, i1, l0, l1) with the float32 arithmetic of the contract; i0, i1 are
    int64, l0, l1 float32."""
    o = torch.arange(2 * n, dtype=torch.float32, device=device)
    r = f32(float(n - 1) / float(2 * n - 1))                   # float32(n - 1) / float32(2n - 1), divided on the host as the launcher does
    s = o * r                                                  # one rounded float32 product per position (r is a float32 value)
    i0 = s.to(torch.int64)                                     # truncation; s >= 0
    l1 = s - i0.to(torch.float32)                              # exact
    l0 = torch.tensor(1.0, dtype=torch.float32, device=device) - l1
    i1 = i0 + (i0 < n - 1).to(torch.int64)
    return i0, i1, l0, l1


def upsample2x_ref64(x):
    """x [..., H, W] float32 -> (ref, S) [..., 2H, 2W] float64:  ref = l0y (l0x a0 + l1x a1) + l1y (l0x b0 + l1x b1)  with the float32
    coordinates of ``axis_coords`` and float64 arithmetic; S is the same expression over magnitudes."""
    H, W = x.shape[-2:]
    y0, y1, l0y, l1y = axis_coords(H, x.device)
    x0, x1, l0x, l1x = axis_coords(W, x.device)
    l0y, l1y = l0y.double()[:, None], l1y.double()[:, None]
    l0x, l1x = l0x.double(), l1x.double()
    x64 = x.to(torch.float64)
    out = []
    for v in (x64, x64.abs()):
        ra, rb = v.index_select(-2, y0), v.index_select(-2, y1)
        ha = l0x * ra.index_select(-1, x0) + l1x * ra.index_select(-1, x1)
        del ra
        hb = l0x * rb.index_select(-1, x0) + l1x * rb.index_select(-1, x1)
        del rb
        out.append(l0y * ha + l1y * hb)
        del ha, hb
    return out[0], out[1]


def axis_matrix(n, device="cpu"):
    """[2n, n] float64: row o holds l0 at i0 and l1 at i1, ADDED, so that the two coincide on the clamped last position."""
    i0, i1, l0, l1 = axis_coords(n, device)
    M = torch.zeros(2 * n, n, dtype=torch.float64, device=device)
    rows = torch.arange(2 * n, device=device)
    M.index_put_((rows, i0), l0.double(), accumulate=True)
    M.index_put_((rows, i1), l1.double(), accumulate=True)
    return M


def upsample2x_backward_ref64(g, H, W):
    """g [P, 2H, 2W] float32 -> (ref, S) [P, H, W] float64: the exact transpose of ``upsample2x_ref64`` with the same float32 weights."""
    assert g.dim() == 3 and g.shape[1:] == (2 * H, 2 * W), tuple(g.shape)
    My, Mx = axis_matrix(H, g.device), axis_matrix(W, g.device)
    g64 = g.to(torch.float64)
    ref = torch.einsum("oy,pow,wx->pyx", My, g64, Mx)
    S = torch.einsum("oy,pow,wx->pyx", My, g64.abs(), Mx)          # the weights are not negative
    return ref, S


# The float32 TWIN of the forward contract: not a reference to compare within a bound, but the kernels' own rounded operations, one by
# one, on the CPU -- lerp2(w0, a, w1, b) = fma(w1, b, rn(w0 a)) with w0 = rn(1 - w1), horizontal first (csrc/misc_kernels.hip; the
# three forward kernels share lerp2, so this is what all of them compute, bit for bit).  It is what answers "can an up-sampled value
# exceed the largest input?" (tests/test_amax_audit_cpu.py): the float64 reference above shows the weights' own excess only (l0 + l1 is
# at most 1 + 2^-25 per axis), not the three roundings of each lerp2.
# Every operation is made in float64 on float32 values and rounded to float32 ONCE: a product of two float32 numbers is exact in
# float64 (48 bits); the fma's sum is rounded to odd in float64 (TwoSum gives the exact error) before the rounding to float32, which
# makes the double rounding the single one (53 >= 24 + 2).

def _rn32(v):
    import numpy as np
    return v.astype(np.float32).astype(np.float64)


def fma32(a, b, c):
    """float32(a * b + c), rounded once, for float64 arrays that hold float32 values."""
    import numpy as np
    t = a * b                                                    # exact
    s = t + c
    bb = s - t
    e = (t - (s - bb)) + (c - bb)                                # TwoSum: t + c = s + e exactly
    fix = (e != 0) & ((s.view(np.int64) & 1) == 0)               # inexact and even: the odd neighbour lies towards e
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return _rn32(s)


def lerp2_32(w0, a, w1, b):
    return fma32(w1, b, _rn32(w0 * a))


def upsample2x_twin32(x):
    """x [..., H, W] float32 numpy array -> [..., 2H, 2W] float32: the forward kernels' arithmetic, operation by operation."""
    import numpy as np
    assert x.dtype == np.float32
    H, W = x.shape[-2:]
    y0, y1, l0y, l1y = [t.numpy() for t in axis_coords(H)]
    x0, x1, l0x, l1x = [t.numpy() for t in axis_coords(W)]
    l0y, l1y = l0y.astype(np.float64)[:, None], l1y.astype(np.float64)[:, None]
    l0x, l1x = l0x.astype(np.float64), l1x.astype(np.float64)
    v = x.astype(np.float64)
    ra, rb = np.take(v, y0, axis=-2), np.take(v, y1, axis=-2)
    ha = lerp2_32(l0x, np.take(ra, x0, axis=-1), l1x, np.take(ra, x1, axis=-1))
    hb = lerp2_32(l0x, np.take(rb, x0, axis=-1), l1x, np.take(rb, x1, axis=-1))
    return lerp2_32(l0y, ha, l1y, hb).astype(np.float32)


# ---- flat Adam --------------------------------------------------------------------------------------------------------------------------

def f32(x):
    """The float32 nearest to x, as a Python float."""
    return torch.tensor(float(x), dtype=torch.float32).item()


def adam_scalars(lr, b1, b2, eps, wd, step):
    """The float32 numbers the kernel works with, as Python floats: what the entry point receives, bc1 and sqrt(bc2) formed in double and
    rounded to float (sstem_adam_step_f32), and the kernel's own 1.f - beta1, 1.f - beta2 and lr / bc1."""
    lr, b1, b2, eps, wd = f32(lr), f32(b1), f32(b2), f32(eps), f32(wd)
    bc1 = f32(1.0 - math.pow(b1, float(step)))
    bc2s = f32(math.sqrt(1.0 - math.pow(b2, float(step))))
    return dict(lr=lr, b1=b1, b2=b2, eps=eps, wd=wd, bc1=bc1, bc2s=bc2s, c1=f32(1.0 - b1), c2=f32(1.0 - b2), step_size=f32(lr / bc1))


def adam_ref64(p, g, m, v, lr, b1, b2, eps, wd, step):
    """One step of torch.optim.Adam (L2 weight decay added to the gradient, no amsgrad) on float32 tensors, in float64 from the float32
    scalars of ``adam_scalars``.  Returns (p', m', v', S_p, S_m, S_v), all float64; the S are described in the module docstring."""
    k = adam_scalars(lr, b1, b2, eps, wd, step)
    p, g, m, v = (t.to(torch.float64) for t in (p, g, m, v))
    gi = g + k["wd"] * p
    A = g.abs() + (k["wd"] * p).abs()
    m1 = m + (gi - m) * k["c1"]
    S_m = m.abs() + k["c1"] * (A + m.abs())
    v1 = k["b2"] * v + k["c2"] * gi * gi
    S_v = k["b2"] * v.abs() + k["c2"] * A * A
    denom = v1.sqrt() / k["bc2s"] + k["eps"]
    p1 = p - k["step_size"] * (m1 / denom)
    T1 = k["step_size"] * (m1 / denom).abs()
    T2 = k["step_size"] * S_m / denom
    T3 = T1 * (math.sqrt(k["c2"]) * A / (k["bc2s"] * denom)) if k["wd"] != 0.0 else torch.zeros_like(T1)
    c = ADAM_P_COUNTS
    S_p = c[0] * p1.abs() + c[1] * T1 + c[2] * T2 + c[3] * T3
    return p1, m1, v1, S_p, S_m, S_v


def adam_inputs(n, generator, device="cpu"):
    """(p, g, m, v) float32 of n elements for the Adam checks: |g|, |m| log-uniform over 1e-9 .. 1e2 with random signs, v log-uniform
    over 1e-18 .. 1e4 (sqrt(v) from far below eps = 1e-8 to far above it), p normal; 1 % of g and, independently, of v exactly zero."""
    def rnd(*a):
        return torch.rand(n, generator=generator, device=device, dtype=torch.float64)

    def logu(lo, hi):
        return torch.pow(10.0, lo + (hi - lo) * rnd())

    def sign():
        return torch.where(rnd() < 0.5, -1.0, 1.0)
    g = logu(-9.0, 2.0) * sign()
    m = logu(-9.0, 2.0) * sign()
    v = logu(-18.0, 4.0)
    g = torch.where(rnd() < 0.01, torch.zeros_like(g), g)
    v = torch.where(rnd() < 0.01, torch.zeros_like(v), v)
    p = torch.randn(n, generator=generator, device=device, dtype=torch.float64)
    return tuple(t.to(torch.float32).contiguous() for t in (p, g, m, v))


# ---- uint8 store ------------------------------------------------------------------------------------------------------------------------

def f32_to_u8_ref(v, clamp01):
    """The conversion rule csrc/misc_kernels.hip states for f32_to_gray_u8: after the optional clamp to [0, 1] (a NaN passes it), multiply
    by 255 in float32, truncate toward zero to a 64-bit integer, keep the low 8 bits (256.0 -> 0, -1.0 -> 255); NaN and |.| >= 9e18 -> 0.
    Integer arithmetic throughout: no float -> uint8 cast of an out-of-range value."""
    assert v.dtype == torch.float32
    p = v
    if clamp01:
        one, zero = torch.ones((), dtype=torch.float32, device=v.device), torch.zeros((), dtype=torch.float32, device=v.device)
        p = torch.where(p > 1.0, one, torch.where(p < 0.0, zero, p))
    t = p * torch.tensor(255.0, dtype=torch.float32, device=v.device)
    ok = (t == t) & (t.abs() < torch.tensor(9.0e18, dtype=torch.float32, device=v.device))
    w = torch.where(ok, t, torch.zeros_like(t)).to(torch.int64)              # in range: the cast truncates toward zero
    return torch.bitwise_and(w, 0xFF).to(torch.uint8)


# ---- the check --------------------------------------------------------------------------------------------------------------------------

def rounding_report(got, ref, S, n):
    """Where ``got`` leaves  |got - ref| <= n * 2^-24 * S + 2^-120  (a NaN or Inf in ``got`` counts as leaving it).
    Returns {"bad": count, "worst": max err / (2^-24 S) over the finite elements, "first": index tuple of the first bad element}."""
    assert got.shape == ref.shape == S.shape, (tuple(got.shape), tuple(ref.shape), tuple(S.shape))
    assert ref.dtype == torch.float64 and S.dtype == torch.float64
    g = got.to(torch.float64)
    finite = torch.isfinite(g)
    err = torch.where(finite, (g - ref).abs(), torch.zeros_like(ref))
    bad = ~finite | (err > n * U * S + ABS_SLACK)
    ratio = err / (U * S + ABS_SLACK)
    rep = {"bad": int(bad.sum().item()), "worst": float(ratio.max().item()) if ratio.numel() else 0.0, "first": None,
           "nonfinite": int((~finite).sum().item())}
    if rep["bad"]:
        flat = int(torch.nonzero(bad.reshape(-1))[0].item())
        idx = []
        for d in reversed(got.shape):
            idx.append(flat % d)
            flat //= d
        rep["first"] = tuple(reversed(idx))
        rep["first_ratio"] = float(ratio[rep["first"]].item())
    return rep


def assert_within_rounding(got, ref, S, n, what):
    """Every element of ``got`` within the derived rounding bound of ``ref``; returns the worst err / (2^-24 S).  The failure message
    carries the index of the first bad element (for planes [P, H, W]: plane, row, column) and its distance from the far edges."""
    rep = rounding_report(got, ref, S, n)
    if rep["bad"]:
        first = rep["first"]
        raise AssertionError(
            "%s: %d of %d elements outside %g * 2^-24 * S (%d not finite); worst err / (2^-24 S) = %.4g; first bad element %s "
            "(from the far edges: %s) at ratio %.4g: got %.9g, reference %.17g"
            % (what, rep["bad"], got.numel(), n, rep["nonfinite"], rep["worst"], list(first),
               [d - 1 - i for d, i in zip(got.shape, first)], rep["first_ratio"], float(got[first].item()), float(ref[first].item())))
    return rep["worst"]
