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
* **BF16** (one piece): both operands at most 8 bits -- families A and B degenerate to one-piece x one-piece ("I").  The id ROUNDS by
  contract ("rounded to bf16 (RNE)", include/sstem_conv.h), so it has two more families whose dense operand needs rounding: (R) a
  dense ``needs_rounding`` input x few-hot small-integer weights, (R') dense ``needs_rounding`` weights x an input that is few-hot
  over pixels and channels.  ``exact_domain("bf16", x, w, rounded=True)`` accepts such a pair: the single piece IS the rounded
  value ``rne_bf16(x)`` and the residual x - piece is dropped by contract, so the reference is the float64 convolution of the two
  rounded operands and the budget is taken over the rounded magnitudes.  Without ``rounded`` a multi-piece operand is still refused.
* **fp32 MFMA, DIRECT, streaming**: exact products, so any operand pair inside the budget: A, B and C.

Generators
----------
``needs_rounding`` draws  s (128 + k + f/4) 2^e  (k in 0..127, f in 0..3, e in -2..2): ten significant bits, of which bf16 keeps
eight, so f selects the rounding class -- exact (f = 0), below half (1), a tie (2; to even: downwards in magnitude for k even, upwards
for k odd), above half (3), and for k = 127, f >= 2 a carry into the next binade.  ``rounding_census`` counts the six classes from
the bit patterns of any fp32 tensor and ``assert_rounding_census`` asks for at least 5 % in each of the first five and two carries
per thousand elements: a randn value is never a tie, so a test on randn data cannot tell round-to-nearest-even from round-half-away
or round-half-up.  ``rounding_store_operands`` makes 8-bit operands (nothing rounds while they are staged) whose SUMS need ten bits:
what a bf16 output store has to round, with the same census asserted of the values before the store.

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
FAMILIES = {"x6": ("A", "B", "C"), "x3": ("A", "B"), "f16x3": ("A", "B"), "bf16": ("I", "R", "R'"), "fp32": ("A", "B", "C")}
ROUNDED_FAMILIES = ("R", "R'")                                   # the dense operand is not a bf16 number: the id rounds it (BF16 only)
Q_ROUNDED = 2.0 ** -2                                            # quantum of a rounded needs_rounding value
CENSUS_CLASSES = ("exact", "below_half", "tie_down", "tie_up", "above_half", "carry")


# ---- round to nearest even, restated on the bit pattern ----------------------------------------------------------------------------------
def _bits(x):
    assert x.dtype == torch.float32
    return x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def _from_bits(u):
    u = torch.where(u >= 2 ** 31, u - 2 ** 32, u)
    return u.to(torch.int32).view(torch.float32)


def rne_bf16(x, mode="rne"):
    """fp32 -> the nearest bf16 number, ties to even, as an fp32 tensor: add 0x7FFF + bit 16 to the bit pattern, clear the low half
    (integer tensor operations only; a NaN stays a NaN).  It restates the contract of include/sstem_conv.h, not the kernel.  The other
    modes are the MUTANTS of tests/test_conv_bf16_exact_cpu.py: "trunc" clears the low half, "away" adds 0x8000 (ties away from
    zero), "up" rounds ties towards +infinity."""
    u = _bits(x)
    if mode == "rne":
        r = u + 0x7FFF + ((u >> 16) & 1)
    elif mode == "trunc":
        r = u
    elif mode == "away":
        r = u + 0x8000
    elif mode == "up":                                            # positive: half rounds up in magnitude; negative: half rounds down
        r = u + torch.where((u >> 31) == 0, torch.full_like(u, 0x8000), torch.full_like(u, 0x7FFF))
    else:
        raise ValueError(mode)
    r = r & 0xFFFF0000
    nan = ((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0)
    r = torch.where(nan, (u & 0xFFFF0000) | 0x00400000, r)
    return _from_bits(r).reshape(x.shape)


def rounding_census(x):
    """How many elements of the fp32 tensor fall into each class of the bf16 rounding (CENSUS_CLASSES), from the bit patterns: the
    dropped half against 0x8000, bit 16 for the direction of a tie; a carry is a value that rounds UP out of an all-ones kept
    mantissa (it is counted in its own class as well)."""
    u = _bits(x)
    low, odd, ones = u & 0xFFFF, ((u >> 16) & 1) == 1, ((u >> 16) & 0x7F) == 0x7F
    tie = low == 0x8000
    up = (low > 0x8000) | (tie & odd)
    counts = [low == 0, (low > 0) & (low < 0x8000), tie & ~odd, tie & odd, low > 0x8000, up & ones]
    return {k: int(c.sum()) for k, c in zip(CENSUS_CLASSES, counts)}


def assert_rounding_census(census, n, what="tensor"):
    """At least 5 % of the n elements in each of the first five classes and two carries per thousand: a condition on the INPUTS."""
    for k in CENSUS_CLASSES[:5]:
        assert census[k] >= 0.05 * n, "%s: only %d of %d elements are of the rounding class %s" % (what, census[k], n, k)
    assert census["carry"] >= 0.002 * n and (n == 0 or census["carry"] >= 1), "%s: only %d carries in %d elements" % (what, census["carry"], n)
    return census


def needs_rounding(shape, gen, exps=(-2, -1, 0, 1, 2)):
    """fp32 values  s (128 + k + f/4) 2^e,  k in 0..127, f in 0..3, e in `exps`, s = +-1, and the census of their six rounding classes,
    which the function ASSERTS (assert_rounding_census) -- once from k and f, once from the bit patterns.  Carries (k = 127, f >= 2)
    are two in 512 draws; where that leaves a tensor short of two per thousand (or of two at all), elements are planted.  The rounded
    values are multiples of Q_ROUNDED 2^(2 + min e) and of magnitude <= 256 * 2^max(e)."""
    n = 1
    for d in shape:
        n *= d
    k = torch.randint(128, (n,), generator=gen)
    f = torch.randint(4, (n,), generator=gen)
    want = min(n, max(2, math.ceil(0.003 * n)))
    short = want - int(((k == 127) & (f >= 2)).sum())
    if short > 0:
        at = torch.randperm(n, generator=gen)[:min(n, 2 * want)]
        at = at[~((k[at] == 127) & (f[at] >= 2))][:short]
        k[at] = 127
        f[at] = 2 + torch.randint(2, (at.numel(),), generator=gen)
    e = torch.tensor(list(exps), dtype=torch.float64)[torch.randint(len(exps), (n,), generator=gen)]
    s = (torch.randint(2, (n,), generator=gen) * 2 - 1).double()
    v = s * (128.0 + k.double() + f.double() / 4.0) * 2.0 ** e
    x = v.float()
    assert torch.equal(x.double(), v)
    tie = f == 2
    planned = {"exact": int((f == 0).sum()), "below_half": int((f == 1).sum()), "tie_down": int((tie & (k % 2 == 0)).sum()),
               "tie_up": int((tie & (k % 2 == 1)).sum()), "above_half": int((f == 3).sum()), "carry": int(((k == 127) & (f >= 2)).sum())}
    census = rounding_census(x)
    assert census == planned, (census, planned)
    assert_rounding_census(census, n, "needs_rounding")
    r = rne_bf16(x)
    assert_quantum(r, Q_ROUNDED * 2.0 ** (2 + min(exps)), "rounded value")
    assert float(r.abs().max()) <= 256.0 * 2.0 ** max(exps) if n else True
    return x.reshape(shape), census


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


def exact_domain(algo_id, x, w, x_bound=None, w_bound=None, rounded=False):
    """The pieces of both operands under `algo_id`, after checking that the id is exact on the pair: every operand is the sum of its
    pieces, and of every dropped product at least one factor is zero everywhere.  Returns (x pieces, w pieces).
    rounded (the "bf16" id only, families R and R'): the id rounds its operands by contract, so the single piece of each operand is
    rne_bf16(operand) -- checked here to be what torch's own cast gives -- and the residual is dropped: the id is exact on the
    ROUNDED pair, which is what the reference and the budget then take."""
    kind, P, kept = KEPT[algo_id]
    if rounded:
        if algo_id != "bf16":
            raise OutsideExactDomain("%s does not round its operands by contract" % algo_id)
        px, pw = [rne_bf16(x)], [rne_bf16(w)]
        for name, t, ps in (("input", x, px), ("weight", w, pw)):
            if not torch.equal(ps[0], t.bfloat16().float()):
                raise OutsideExactDomain("bf16: the rounded %s is not torch's own bf16 cast" % name)
        return px, pw
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
    # the rounded families: dense needs_rounding values (rounded: multiples of 2^-2, magnitude <= 1024) against six small integers per
    # output sum: S <= 6 x 3 x 1024 + 3 = 2^16.2 q, far inside the budget
    ("bf16", "R"): ("round", "ints", [(3.0, 1.0, 2.0, 1.0, 3.0, 2.0), (1.0, 2.0, 3.0, 1.0, 1.0, 2.0)], None),
    ("bf16", "R'"): ("round", "ints", [(3.0, 1.0, 2.0, 1.0, 3.0, 2.0), (1.0, 2.0, 3.0, 1.0, 1.0, 2.0)], None),
}
for _f in ("A", "B", "C"):
    FAMILY_SPECS[("fp32", _f)] = FAMILY_SPECS[("x6", _f)]


def few_hot_input(shape, per_sum, gen, must_hit=None):
    """An [N, C, H, W] input that is few-hot over pixels AND channels: about `per_sum` entries of +-{1, 2, 3} inside the 9 C values a
    3 x 3 output sum reads, at random positions of every image (one of them inside `must_hit`, a bool tensor over (C, H, W)), and one
    entry on every special_pixels position, walking through the channels from the last one down."""
    N, C, H, W = shape
    entries = min(C * H * W, max(1, math.ceil(per_sum * H * W / 9.0)))
    x, _ = few_hot(N, (C, H, W), entries, gen, "ints", [float(1 + i % 3) for i in range(entries)], must_hit)
    for i, (n, y, xx) in enumerate(special_pixels(N, H, W)):
        x[n, C - 1 - i % C, y, xx] = float(1 + i % 3) * (1 - 2 * (i % 2))
    return x


def _rounded_family_operands(family, dense_shape, nout, domain, gen, seed, must_hit, pixels, exps):
    mags = FAMILY_SPECS[("bf16", family)][2]
    m = list(mags[seed % len(mags)])
    if pixels is not None:                                        # weight gradient: (input, gradient [N, nout, H, W])
        N, H, W = pixels
        m = m[:N * H * W]
        def on_every_special_pixel(hot):                          # (few_hot_pixels reaches two of them per channel: too few with 8 channels)
            for i, (n, y, xx) in enumerate(special_pixels(N, H, W)):
                hot[n, i % hot.shape[1], y, xx] = float(1 + i % 3) * (1 - 2 * (i % 2))
            return hot
        if family == "R":
            dense, _ = needs_rounding(dense_shape, gen, exps)
            hot, _ = few_hot_pixels(nout, N, H, W, len(m), gen, "ints", m)
            return dense, on_every_special_pixel(hot), Q_ROUNDED
        dense, _ = needs_rounding((N, nout, H, W), gen, exps)
        hot, _ = few_hot_pixels(dense_shape[1], N, H, W, len(m), gen, "ints", m)
        return on_every_special_pixel(hot), dense, Q_ROUNDED
    if family == "R":
        dense, _ = needs_rounding(dense_shape, gen, exps)
        room = int(torch.tensor(domain).prod())
        hot, _ = few_hot(nout, domain, min(len(m), room), gen, "ints", m[:room], must_hit)
        return dense, hot, Q_ROUNDED
    dense, _ = needs_rounding((nout,) + tuple(domain), gen, exps)
    chan = None
    if must_hit is not None:                                      # must_hit is over the weights' (Cin, 3, 3): the same channels of the input
        chan = must_hit.reshape(must_hit.shape[0], -1).any(1).view(-1, 1, 1).expand(dense_shape[1:]).contiguous()
    return few_hot_input(dense_shape, len(m), gen, chan), dense, Q_ROUNDED


def family_operands(algo_id, family, dense_shape, nout, domain, seed, must_hit=None, pixels=None, exps=(-2, -1, 0, 1, 2)):
    """One operand pair of `family` under `algo_id`: (dense, few_hot, q).  The dense operand has `dense_shape`; the few-hot one is
    [nout, *domain] (weights: domain = (Cin, 3, 3)), or [N, nout, H, W] gradient pixels when pixels = (N, H, W).  In families A, C
    and I the dense operand is the multi-piece one; in B the few-hot one is.
    The rounded families of the "bf16" id return (input-side operand [dense_shape], weight-side operand, Q_ROUNDED): under R the
    input is the dense needs_rounding one (exponents `exps`) and the other few-hot small integers; under R' the weight-side operand
    ([nout, *domain], or the [N, nout, H, W] gradient) is dense and the input few-hot (few_hot_input / few_hot_pixels)."""
    if family not in FAMILIES[algo_id]:
        raise OutsideExactDomain("%s is not exact on family %s" % (algo_id, family))
    dk, fk, mags, entries = FAMILY_SPECS[(algo_id, family)]
    gen = torch.Generator().manual_seed(seed)
    if family in ROUNDED_FAMILIES:
        return _rounded_family_operands(family, dense_shape, nout, domain, gen, seed, must_hit, pixels, exps)
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


# ---- operands for the bf16 OUTPUT store ----------------------------------------------------------------------------------------------------
# the second (and third) weight of an output channel is its first one times 2^-j, j walking through this list: two channels in three
# put the sum on the quarter grid of its last kept bit (where the ties are), the others put it anywhere between
STORE_SHIFTS = (1, 2, 9, 1, 2, 5, 2, 1, 7, 2, 3, 1, 2, 4, 1, 2, 6, 2, 1, 8)
Q_STORE = 2.0 ** -9


def rounding_store_operands(shape, seed, act=2, slope=0.25, tries=24, with_scale=True):
    """Operands whose EXACT fp32 result needs more than 8 significant bits, so that a bf16 output store has something to round, while
    nothing rounds on the way in: inputs +-(128 + k) (8 bits; k = 127 on one element in twenty more than by chance, for the carries),
    two-hot (even channels) or three-hot weights +-1, +-2^-j, +-2^-j' (STORE_SHIFTS), a bias on the grid 2^-2, 2^-3 or 2^-4, a scale
    in {0.5, 1, 2} (None without `with_scale`).  Returns (x, w, bias, scale, pre, census): `pre` is epilogue_ref64 of the float64 convolution -- the value BEFORE
    the store, every stage an fp32 number --, and the reference of the stored tensor is rne_bf16(pre.float()).  The census of `pre`
    is asserted (assert_rounding_census); seed and bias grid are stepped until it holds."""
    N, Cin, H, W, Cout = shape
    last = None
    for t in range(tries):
        gen = torch.Generator().manual_seed(seed + 1009 * t)
        k = torch.randint(128, (N, Cin, H, W), generator=gen)
        k = torch.where(torch.rand(N, Cin, H, W, generator=gen) < 1.0 / 20.0, torch.full_like(k, 127), k)
        x = ((torch.randint(2, k.shape, generator=gen) * 2 - 1) * (128 + k)).float()
        w = torch.zeros(Cout, Cin * 9)
        for co in range(Cout):
            pos = torch.randperm(Cin * 9, generator=gen)[:3 if co % 2 else 2]
            j = (0, STORE_SHIFTS[(co + t) % len(STORE_SHIFTS)], STORE_SHIFTS[(co + t + 7) % len(STORE_SHIFTS)])
            for i, p in enumerate(pos.tolist()):
                w[co, p] = float(1 - 2 * int(torch.randint(2, (1,), generator=gen))) * 2.0 ** -j[i]
        w = w.reshape(Cout, Cin, 3, 3)
        grid = 2.0 ** -(2 + t % 3)
        bias = (torch.randint(-8, 9, (Cout,), generator=gen).double() * grid).float()
        scale = _pick((Cout,), [0.5, 1.0, 2.0], gen).float() if with_scale else None
        for name, v in (("input", x), ("weight", w)):
            assert torch.equal(rne_bf16(v), v), "%s: not a bf16 number" % name
        assert_quantum(bias, Q_STORE, "bias")
        assert_exactly_summable(forward_terms_abs([x], [w], bias), Q_STORE)
        pre = epilogue_ref64(assert_fp32_number(conv_ref64(x, w, bias)), scale, None, act, slope)
        census = rounding_census(pre.float())
        try:
            assert_rounding_census(census, pre.numel(), "values before the bf16 store")
        except AssertionError as e:
            last = e
            continue
        return x, w, bias, scale, pre, census
    raise last
