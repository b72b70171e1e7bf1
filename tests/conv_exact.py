"""Exactly summable inputs for the convolution kernels (test infrastructure only; torch, any device, nothing shared with the kernels).

A GEMM-shaped kernel cannot be held to a per-element rounding bound the way the sepconv kernels are (tests/sepconv_ref64.py): a 3 x 3
convolution sums K = 9 Cin products, and n 2^-24 S at K = 4608 is 130 times looser than the 2e-5 the suite already asserts.  What does
work is an input whose terms sum EXACTLY IN ANY ORDER: then every kernel that forms every product its id promises returns the float64
reference bit for bit, at every element, and a kernel that drops, misplaces or mis-scales a piece cannot.

The budget rule
---------------
Let every term of every output sum be an integer multiple of a quantum ``q`` (a power of two), and let ``S`` be the sum of the terms'
magnitudes.  Every partial sum, over any subset and in any order, is then a multiple of q of magnitude <= S.  With S <= 2^24 q it is
an integer below 2^24 times a power of two: an fp32 number, added without rounding (fp32 MFMA accumulators and the plain fp32 adds of
the K-slice and slab reduces alike).  ``assert_exactly_summable(S, q)`` asks for S <= 2^23 q: one bit is left for the epilogue
(bias, folded affine with a scale in {0.5, 1, 2}, LeakyReLU with slope 0.25, residual times 0.5), whose operands are counted in S as
well and whose stages ``epilogue_ref64`` checks to be fp32 numbers one by one.  The split ids sum PIECE products, so S is taken over
the pieces' own magnitudes (|h| + |m| + |l| can exceed |x|: the pieces alternate in sign).  This is a condition on the INPUTS, checked
before a kernel's output is looked at; it is no tolerance.

Exact domain per id (include/sstem_conv.h, csrc/conv_split_common.h)
-------------------------------------------------------------------
``split_pieces<P>`` makes p_0 = bf16(x), p_1 = bf16(x - p_0), p_2 = bf16(x - p_0 - p_1) (round to nearest even, the subtractions
exact); ``split_pieces_f16`` makes h0 = fp16(x s), h1 = fp16(x s - h0) with s = 2^(141 - e), e the biased exponent of the tensor's
bound.  A kernel keeps the products listed below and drops the others, so its result is x . w exactly iff the pieces add up to the
value AND no dropped product is non-zero; ``exact_domain`` computes the pieces with torch's own casts and refuses an operand pair that
populates a dropped product (``OutsideExactDomain``).

* **X6** (three bf16 pieces; kept: pa + pb <= 2, i.e. hh hm mh hl lh mm).  Families: (A) three-piece input x one-piece weight (at most
  8 significant bits); (B) the operands swapped; (C) two-piece x two-piece, the only one that populates m.m.  Three-piece x two-piece
  populates the dropped m.l / l.m and is refused.
* **F16X3** (two fp16 pieces; kept: h0g0 h0g1 h1g0).  Families: (A) two-piece input (at most 22 bits) x one-piece weight (at most 11
  bits); (B) swapped.  Two-piece x two-piece populates the dropped h1g1.  All values stay within 18 binades of the tensor's bound
  (the pieces then add up to the value, which exact_domain checks); the amax word is the true maximum.
* **X3** (two bf16 pieces; kept: hh hm mh).  (A) input of at most 16 bits x weight of at most 8 bits; (B) swapped.
* **BF16** (one piece): both operands at most 8 bits -- families A and B degenerate to one-piece x one-piece ("I").
* **fp32 MFMA, DIRECT, streaming**: exact products, so any operand pair inside the budget: A, B and C.

Generators
----------
Multi-piece values are  a + b 2^-8 + c 2^-19  (three bf16 pieces),  a + b 2^-8  (two) and  a + c 2^-shift, shift = 12  (two fp16
pieces), a in +-{2, 3}, b and c in +-{1, 2, 3}: at most 21 significant bits.  Which pieces a value populates depends on where the
roundings fall (c 2^-16 instead of c 2^-19 disappears into the second bf16 piece on two thirds of the elements), so ``multi_piece``
ASSERTS that every piece is non-zero on at least 90 % of the elements instead of assuming it (about one value in twelve of the bf16
forms loses b 2^-8 to the first piece's rounding; such elements are drawn again first).  The partner operand is few-hot: a
handful of entries per output sum, at random positions that differ from one output channel to the next (``few_hot``), small integers
(one piece) or multi-piece values, the count chosen so that the budget holds (``FAMILY_SPECS``).

References, all in float64: ``conv_ref64`` (k x k "same" convolution as k^2 shifted einsums), ``conv_dgrad_ref64``,
``conv_wgrad_ref64`` (weight and bias gradient), ``convT_ref64`` / ``convT_dgrad_ref64`` / ``convT_wgrad_ref64``
(ConvTranspose k3 s2 p1 op1), ``epilogue_ref64``, ``pool2x2_ref64``.
"""
import math

import torch

Q_BF16_3 = 2.0 ** -19          # quantum of a + b 2^-8 + c 2^-19
Q_BF16_2 = 2.0 ** -8
F16_SHIFT = 12
BUDGET_BITS = 23


class OutsideExactDomain(AssertionError):
    """The operand pair populates a product the id drops, or its pieces do not add up to the value."""


# kept (input piece, weight piece) products per id; "fp32": no pieces, every product exact
KEPT = {
    "x6": ("bf16", 3, [(0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1)]),
    "x3": ("bf16", 2, [(0, 0), (0, 1), (1, 0)]),
    "f16x3": ("f16", 2, [(0, 0), (0, 1), (1, 0)]),
    "bf16": ("bf16", 1, [(0, 0)]),
    "fp32": (None, 1, [(0, 0)]),
}
FAMILIES = {"x6": ("A", "B", "C"), "x3": ("A", "B"), "f16x3": ("A", "B"), "bf16": ("I",), "fp32": ("A", "B", "C")}


# ---- pieces, as torch's own casts make them --------------------------------------------------------------------------------------------
def pieces_bf16(x, P, third_from_first_residual=False):
    """split_pieces<P>: p_k = bf16(x - p_0 - .. - p_{k-1}).  third_from_first_residual: the mutant that rounds the third piece from
    x - p_0 instead of subtracting p_1 first (tests/test_conv_exact_cpu.py)."""
    assert x.dtype == torch.float32
    out, r = [], x
    for p in range(P):
        src = (x - out[0]) if (third_from_first_residual and p == 2) else r
        o = src.bfloat16().float()
        out.append(o)
        r = r - o
    return out


def amax_exponent(bound):
    """Biased exponent of the bound, clamped as csrc/conv_split_common.h clamps it."""
    bound = float(bound)
    if bound == 0.0 or not math.isfinite(bound):
        return 141 if bound != 0.0 else 16
    e = math.frexp(bound)[1] + 126
    return min(max(e, 16), 250)


def pieces_f16(x, bound=None, scale_binades_off=0):
    """split_pieces_f16 under s = 2^(141 - e): the two pieces, de-scaled (a power of two: exact).  scale_binades_off: the mutant whose
    second piece is taken out of the sum with a scale one binade off."""
    assert x.dtype == torch.float32
    bound = float(x.abs().max()) if bound is None else float(bound)
    s = 2.0 ** (141 - amax_exponent(bound))
    xs = x * s
    h0 = xs.half().float()
    h1 = (xs - h0).half().float()
    return [h0 / s, h1 / (s * 2.0 ** scale_binades_off)]


def pieces_of(algo_id, x, bound=None):
    kind, P, _ = KEPT[algo_id]
    if kind is None:
        return [x]
    return pieces_f16(x, bound) if kind == "f16" else pieces_bf16(x, P)


def exact_domain(algo_id, x, w, x_bound=None, w_bound=None):
    """The pieces of both operands under `algo_id`, after checking that the id is exact on the pair: every operand is the sum of its
    pieces, and of every dropped product at least one factor is zero everywhere.  Returns (x pieces, w pieces)."""
    kind, P, kept = KEPT[algo_id]
    px, pw = pieces_of(algo_id, x, x_bound), pieces_of(algo_id, w, w_bound)
    for name, t, ps in (("input", x, px), ("weight", w, pw)):
        if not torch.equal(sum(p.double() for p in ps), t.double()):
            raise OutsideExactDomain("%s: the %s is not the sum of its %d pieces" % (algo_id, name, len(ps)))
    for a in range(len(px)):
        for b in range(len(pw)):
            if (a, b) not in kept and bool(px[a].any()) and bool(pw[b].any()):
                raise OutsideExactDomain("%s drops the product (input piece %d) x (weight piece %d), and both are populated" % (algo_id, a, b))
    return px, pw


def piece_magnitudes(ps):
    """sum_p |piece_p| in float64: what an operand contributes to the budget."""
    return sum(p.double().abs() for p in ps)


def assert_quantum(t, q, what="tensor"):
    """Every element an integer multiple of q."""
    r = t.double() / q
    assert torch.equal(r, r.round()), "%s: not a multiple of 2^%d everywhere" % (what, round(math.log2(q)))


def assert_exactly_summable(terms_abs_sum, q):
    """terms_abs_sum: float64 sum of the magnitudes of the terms of every output element (pieces' own magnitudes, epilogue operands
    included).  Asserts S <= 2^23 q at every element -- a condition on the inputs -- and returns max S / q."""
    assert terms_abs_sum.dtype == torch.float64
    worst = float(terms_abs_sum.max()) / q if terms_abs_sum.numel() else 0.0
    assert worst <= 2.0 ** BUDGET_BITS, "sum|terms| / q = %.4g exceeds 2^%d: the case is not exactly summable" % (worst, BUDGET_BITS)
    return worst


def assert_fp32_number(ref, what="reference"):
    """The float64 reference is its own fp32 rounding."""
    assert ref.dtype == torch.float64
    assert torch.equal(ref.float().double(), ref), "%s: not representable in fp32" % what
    return ref


# ---- generators ------------------------------------------------------------------------------------------------------------------------
def _pick(shape, values, gen):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(len(values), shape, generator=gen)]


def _draw(shape, kind, gen, low_shift):
    a = _pick(shape, [-3.0, -2.0, 2.0, 3.0], gen)
    small = [-3.0, -2.0, -1.0, 1.0, 2.0, 3.0]
    if kind == "bf16x3":
        sh = 19 if low_shift is None else low_shift
        return a + _pick(shape, small, gen) * 2.0 ** -8 + _pick(shape, small, gen) * 2.0 ** -sh, 2.0 ** -sh, ("bf16", 3)
    if kind == "bf16x2":
        return a + _pick(shape, small, gen) * 2.0 ** -8, Q_BF16_2, ("bf16", 2)
    if kind == "f16x2":
        sh = F16_SHIFT if low_shift is None else low_shift
        return a + _pick(shape, small, gen) * 2.0 ** -sh, 2.0 ** -sh, ("f16", 2)
    if kind == "int":
        return _pick(shape, small, gen), 1.0, None
    if kind == "int2":
        return _pick(shape, [-2.0, -1.0, 1.0, 2.0], gen), 1.0, None
    raise ValueError(kind)


def multi_piece(shape, kind, gen, low_shift=None, min_populated=0.9, redraw=True):
    """kind "bf16x3": a + b 2^-8 + c 2^-low_shift (19); "bf16x2": a + b 2^-8; "f16x2": a + c 2^-low_shift (12); "int": +-{1, 2, 3};
    "int2": +-{1, 2}.  Returns (float32 tensor, quantum).  About one value in twelve of the bf16 forms rounds so that a piece comes
    out empty (b 2^-8 absorbed by the first piece's rounding): with `redraw` such elements are drawn again, a few times.  Either way
    the function ASSERTS that the value is an fp32 number, the sum of its pieces, and that each piece is non-zero on at least
    min_populated of the elements."""
    v, q, ps = _draw(shape, kind, gen, low_shift)

    def split(t):
        return pieces_f16(t.float(), 3.0 + 3.0 * q) if ps[0] == "f16" else pieces_bf16(t.float(), ps[1])
    if ps is not None and redraw:
        for _ in range(8):
            empty = torch.zeros(v.shape, dtype=torch.bool)
            for p in split(v):
                empty |= p == 0
            if not bool(empty.any()):
                break
            v = torch.where(empty, _draw(shape, kind, gen, low_shift)[0], v)
    x = v.float()
    assert torch.equal(x.double(), v), "%s: the value is not an fp32 number" % kind
    if ps is not None:
        pieces = split(v)
        assert torch.equal(sum(p.double() for p in pieces), v), "%s: the pieces do not add up to the value" % kind
        for i, p in enumerate(pieces):
            frac = float((p != 0).double().mean()) if p.numel() else 1.0
            assert frac >= min_populated, "%s: piece %d is non-zero on %.1f %% of the elements only" % (kind, i, 100 * frac)
    return x, q


def few_hot(nout, domain, entries, gen, kind="ints", mags=None, must_hit=None):
    """[nout, *domain] zeros with `entries` non-zero values per output index at distinct random positions that differ between the
    output indices.  kind "ints": magnitudes `mags` (one per entry) with random signs; otherwise a multi_piece kind.  must_hit: a bool
    tensor over `domain`; one entry of every output index lands inside it (the last K chunk, say)."""
    D = 1
    for d in domain:
        D *= d
    assert entries <= D
    score = torch.rand(nout, D, generator=gen)
    if must_hit is not None:
        allowed = torch.nonzero(must_hit.reshape(-1)).reshape(-1)
        assert allowed.numel() > 0
        pick = allowed[torch.randint(allowed.numel(), (nout,), generator=gen)]
        score[torch.arange(nout), pick] += 10.0
    pos = score.topk(entries, dim=1).indices
    if kind == "ints":
        mags = [1.0] * entries if mags is None else mags
        assert len(mags) == entries
        vals = torch.tensor(mags, dtype=torch.float32).repeat(nout, 1) * (torch.randint(2, (nout, entries), generator=gen) * 2 - 1).float()
        q = 1.0
    else:
        vals, q = multi_piece((nout, entries), kind, gen)
    out = torch.zeros(nout, D)
    out.scatter_(1, pos, vals)
    return out.reshape((nout,) + tuple(domain)), q


def special_pixels(N, H, W):
    """Pixels of an [N, H, W] gradient where a weight-gradient kernel's 2-row x 32-column tiles go wrong first: the corners and edges
    of the first and the last image, both rows of the first and the last 2-row tile, columns 31 and 32 (a tile seam) where they exist."""
    ys = sorted({0, 1, H // 2, max(H - 2, 0), H - 1})
    xs = sorted({0, 1, min(31, W - 1), min(32, W - 1), W // 2, max(W - 2, 0), W - 1})
    return [(n, y, x) for n in sorted({0, N - 1}) for y in ys for x in xs]


def few_hot_pixels(nout, N, H, W, entries, gen, kind="ints", mags=None):
    """few_hot over the pixels of [N, H, W] -> [N, nout, H, W]: two entries of every channel sit on special_pixels (walked through
    channel by channel), the others at random."""
    t, q = few_hot(nout, (N, H, W), entries, gen, kind, mags)
    vals = t.reshape(nout, -1)
    sp = special_pixels(N, H, W)
    out = torch.zeros(nout, N * H * W)
    for c in range(nout):
        v = vals[c][vals[c] != 0]
        pos = torch.nonzero(vals[c]).reshape(-1).tolist()
        forced = []
        for k in range(min(2, entries)):
            n, y, x = sp[(2 * c + k) % len(sp)]
            forced.append((n * H + y) * W + x)
        chosen = list(dict.fromkeys(forced + pos))[:entries]
        out[c, torch.tensor(chosen)] = v[:len(chosen)]
    return out.reshape(nout, N, H, W).permute(1, 0, 2, 3).contiguous(), q


# what each family gives the DENSE operand and the FEW-HOT one, per piece format: (dense kind, few-hot kind, few-hot magnitudes or
# None, entries).  The entry counts keep  entries x max(sum|dense pieces|) x max(sum|few-hot pieces|) + 3 (epilogue operands: bias,
# shift and residual of magnitude <= 1 each)  inside 2^23 q; assert_exactly_summable checks the tensors themselves.
#   bf16 x 3, q = 2^-19, budget 16:   A: sum|w| = 4 x 3.04 = 12.2;   B: 2 entries x 2 x 3.04 = 12.2
#   bf16 x 2 x bf16 x 2, q = 2^-16, budget 128:   C: 8 entries x 3.02^2 = 73
#   bf16 x 2, q = 2^-8 (budget 2^15);  fp16 x 2, q = 2^-12 (budget 2^11):   8 entries x 3.01 x 2 = 48
FAMILY_SPECS = {
    ("x6", "A"): ("bf16x3", "ints", [(2.0, 1.0, 1.0), (1.0, 1.0, 1.0, 1.0)], None),
    ("x6", "B"): ("int2", "bf16x3", None, 2),
    ("x6", "C"): ("bf16x2", "bf16x2", None, 8),
    ("x3", "A"): ("bf16x2", "ints", [(2.0, 1.0, 2.0, 1.0, 1.0, 2.0, 1.0, 1.0)], None),
    ("x3", "B"): ("int", "bf16x2", None, 8),
    ("f16x3", "A"): ("f16x2", "ints", [(2.0, 1.0, 2.0, 1.0, 1.0, 2.0, 1.0, 1.0)], None),
    ("f16x3", "B"): ("int", "f16x2", None, 8),
    ("bf16", "I"): ("int", "ints", [(2.0, 1.0, 2.0, 1.0, 1.0, 2.0, 1.0, 1.0)], None),
}
for _f in ("A", "B", "C"):
    FAMILY_SPECS[("fp32", _f)] = FAMILY_SPECS[("x6", _f)]


def family_operands(algo_id, family, dense_shape, nout, domain, seed, must_hit=None, pixels=None):
    """One operand pair of `family` under `algo_id`: (dense, few_hot, q).  The dense operand has `dense_shape`; the few-hot one is
    [nout, *domain] (weights: domain = (Cin, 3, 3)), or [N, nout, H, W] gradient pixels when pixels = (N, H, W).  In families A, C
    and I the dense operand is the multi-piece one; in B the few-hot one is."""
    if family not in FAMILIES[algo_id]:
        raise OutsideExactDomain("%s is not exact on family %s" % (algo_id, family))
    dk, fk, mags, entries = FAMILY_SPECS[(algo_id, family)]
    gen = torch.Generator().manual_seed(seed)
    dense, qd = multi_piece(dense_shape, dk, gen)
    room = pixels[0] * pixels[1] * pixels[2] if pixels is not None else int(torch.tensor(domain).prod())
    if mags is not None:
        m = list(mags[seed % len(mags)])[:room]
        entries = len(m)
    else:
        m, entries = None, min(entries, room)
    if pixels is not None:
        hot, qh = few_hot_pixels(nout, pixels[0], pixels[1], pixels[2], entries, gen, fk, m)
    else:
        hot, qh = few_hot(nout, domain, entries, gen, fk, m, must_hit)
    return dense, hot, qd * qh


def epilogue_operands(cout, out_shape, q, seed, residual=False):
    """bias and shift: multiples of q of magnitude <= 1; scale in {0.5, 1, 2}; residual: multiples of q of magnitude <= 1."""
    gen = torch.Generator().manual_seed(seed + 7919)
    step = max(q, 2.0 ** -20)                            # (a coarser power of two is a multiple of q as well)
    steps = max(1, int(1.0 / step))

    def mult(shape):
        return (torch.randint(-steps, steps + 1, shape, generator=gen).double() * step).float()
    bias, shift = mult((cout,)), mult((cout,))
    assert_quantum(bias, q, "bias"); assert_quantum(shift, q, "shift")
    scale = _pick((cout,), [0.5, 1.0, 2.0], gen).float()
    res = mult(tuple(out_shape)) if residual else None
    return bias, scale, shift, res


# ---- float64 references ------------------------------------------------------------------------------------------------------------------
def _shifted(x, dy, dx):
    """x[..., y + dy, x + dx] with zeros outside (x: [N, C, H, W])."""
    N, C, H, W = x.shape
    out = torch.zeros_like(x)
    ys0, ys1 = max(0, -dy), min(H, H - dy)
    xs0, xs1 = max(0, -dx), min(W, W - dx)
    if ys0 < ys1 and xs0 < xs1:
        out[:, :, ys0:ys1, xs0:xs1] = x[:, :, ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx]
    return out


def conv_ref64(x, w, bias=None):
    """out[n,co,y,x] = bias[co] + sum_{ci,ky,kx} w[co,ci,ky,kx] in[n,ci,y+ky-p,x+kx-p], p = (k-1)/2: k^2 shifted einsums in float64."""
    x, w = x.double(), w.double()
    k = w.shape[2]
    p = (k - 1) // 2
    out = torch.zeros(x.shape[0], w.shape[0], x.shape[2], x.shape[3], dtype=torch.float64, device=x.device)
    for ky in range(k):
        for kx in range(w.shape[3]):
            out += torch.einsum("oc,nchw->nohw", w[:, :, ky, kx], _shifted(x, ky - p, kx - (w.shape[3] - 1) // 2))
    if bias is not None:
        out += bias.double().view(1, -1, 1, 1)
    return out


def conv_dgrad_ref64(g, w):
    """grad_in[n,ci,y,x] = sum_{co,ky,kx} g[n,co,y-ky+p,x-kx+p] w[co,ci,ky,kx]."""
    g, w = g.double(), w.double()
    k = w.shape[2]
    p = (k - 1) // 2
    out = torch.zeros(g.shape[0], w.shape[1], g.shape[2], g.shape[3], dtype=torch.float64, device=g.device)
    for ky in range(k):
        for kx in range(k):
            out += torch.einsum("oc,nohw->nchw", w[:, :, ky, kx], _shifted(g, p - ky, p - kx))
    return out


def conv_wgrad_ref64(x, g, k=3):
    """gw[co,ci,ky,kx] = sum_{n,y,x} g[n,co,y,x] in[n,ci,y+ky-p,x+kx-p];  gb[co] = sum_{n,y,x} g[n,co,y,x]."""
    x, g = x.double(), g.double()
    p = (k - 1) // 2
    gw = torch.zeros(g.shape[1], x.shape[1], k, k, dtype=torch.float64, device=x.device)
    for ky in range(k):
        for kx in range(k):
            gw[:, :, ky, kx] = torch.einsum("nohw,nchw->oc", g, _shifted(x, ky - p, kx - p))
    return gw, g.sum((0, 2, 3))


def convT_ref64(x, w, bias=None):
    """ConvTranspose2d(k3, s2, p1, output_padding 1), w [Cin,Cout,3,3]: out[n,co,2y-1+ky,2x-1+kx] += in[n,ci,y,x] w[ci,co,ky,kx]."""
    x, w = x.double(), w.double()
    N, Cin, H, W = x.shape
    big = torch.zeros(N, w.shape[1], 2 * H + 2, 2 * W + 2, dtype=torch.float64, device=x.device)      # index + 1
    for ky in range(3):
        for kx in range(3):
            big[:, :, ky:ky + 2 * H:2, kx:kx + 2 * W:2] += torch.einsum("co,nchw->nohw", w[:, :, ky, kx], x)
    out = big[:, :, 1:2 * H + 1, 1:2 * W + 1].clone()
    if bias is not None:
        out += bias.double().view(1, -1, 1, 1)
    return out


def _padded_grad(g):
    N, C, H2, W2 = g.shape
    big = torch.zeros(N, C, H2 + 2, W2 + 2, dtype=torch.float64, device=g.device)
    big[:, :, 1:H2 + 1, 1:W2 + 1] = g.double()
    return big


def convT_dgrad_ref64(g, w):
    """grad_in[n,ci,y,x] = sum_{co,ky,kx} g[n,co,2y-1+ky,2x-1+kx] w[ci,co,ky,kx]."""
    w = w.double()
    big = _padded_grad(g)
    H, W = g.shape[2] // 2, g.shape[3] // 2
    out = torch.zeros(g.shape[0], w.shape[0], H, W, dtype=torch.float64, device=g.device)
    for ky in range(3):
        for kx in range(3):
            out += torch.einsum("co,nohw->nchw", w[:, :, ky, kx], big[:, :, ky:ky + 2 * H:2, kx:kx + 2 * W:2])
    return out


def convT_wgrad_ref64(x, g):
    """gw[ci,co,ky,kx] = sum_{n,y,x} in[n,ci,y,x] g[n,co,2y-1+ky,2x-1+kx];  gb[co] = sum g[n,co]."""
    x = x.double()
    big = _padded_grad(g)
    H, W = x.shape[2], x.shape[3]
    gw = torch.zeros(x.shape[1], g.shape[1], 3, 3, dtype=torch.float64, device=x.device)
    for ky in range(3):
        for kx in range(3):
            gw[:, :, ky, kx] = torch.einsum("nchw,nohw->co", x, big[:, :, ky:ky + 2 * H:2, kx:kx + 2 * W:2])
    return gw, g.double().sum((0, 2, 3))


def epilogue_ref64(acc, scale=None, shift=None, act=0, slope=0.0, residual=None, res_scale=1.0):
    """(act((conv + bias) scale + shift) + residual) res_scale on the float64 sum `acc` (bias already inside), every stage checked to
    be an fp32 number -- so a kernel may fuse or not fuse its multiply-adds as it likes."""
    v = assert_fp32_number(acc, "conv + bias")
    c = lambda t: t.double().view(1, -1, 1, 1)           # noqa: E731
    if scale is not None:
        v = assert_fp32_number(v * c(scale), "scaled sum")
    if shift is not None:
        v = assert_fp32_number(v + c(shift), "shifted sum")
    if act == 1:
        v = torch.where(v > 0, v, torch.zeros_like(v))
    elif act == 2:
        v = assert_fp32_number(torch.where(v > 0, v, v * slope), "activation")
    if residual is not None:
        v = assert_fp32_number(v + residual.double(), "sum with the residual")
        v = assert_fp32_number(v * res_scale, "scaled residual sum")
    return v


def pool2x2_ref64(v, kind):
    """kind 1: nn.MaxPool2d(2); 2: nn.AvgPool2d(2), in float64."""
    a, b, c, d = v[:, :, 0::2, 0::2], v[:, :, 0::2, 1::2], v[:, :, 1::2, 0::2], v[:, :, 1::2, 1::2]
    if kind == 1:
        return torch.maximum(torch.maximum(a, b), torch.maximum(c, d))
    return (a + b + c + d) * 0.25


def forward_terms_abs(px, pw, bias=None, scale=None, shift=None, residual=None, ref=conv_ref64):
    """S of a forward-shaped launch: the reference on the operands' piece magnitudes + |bias| + |shift| + |residual|.  A scale of 2
    doubles sums and quantum alike and is covered by the spare bit (module docstring)."""
    S = ref(piece_magnitudes(px), piece_magnitudes(pw))
    if bias is not None:
        S = S + bias.double().abs().view(1, -1, 1, 1)
    if shift is not None:
        S = S + shift.double().abs().view(1, -1, 1, 1)
    if residual is not None:
        S = S + residual.double().abs()
    return S
