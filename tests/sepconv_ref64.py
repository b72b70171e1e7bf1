"""Float64 reference of the sepconv operations for every-pixel checks (test infrastructure only; torch, any device).

Written as plain code that shares nothing with the kernels: replication padding by ``F.pad`` and 51 x 51 shifted multiply-adds on
float64 tensors, one shifted slice of the padded plane per tap pair.  On the GPU it costs a few seconds at 8 x 1024 x 1024, so the
kernels can be compared at EVERY pixel of the shapes they run in production instead of on three crops.

    apply_ref64(g1, g2, k1v, k1h, k2v, k2h)  -> (ref, S)            model_interp.py:90-97 on planes [B,1,H,W]
    forward_ref64(inp, ver, hor)             -> (ref, S)            the op on padded frames [B,C,H+50,W+50], any C
    backward_ref64(grad, inp, ver, hor)      -> (gv, gh, S_gv, S_gh)   the formulas of oracle/sepconv_numpy.py

Coefficients are [B,51,H,W], float32 or bfloat16 (widened exactly), contiguous or not; a blocked tensor [B,H,T,51,64] is handed over
as its view ``kb.permute(0, 3, 1, 2, 4)`` = [B,51,H,T,64] (no copy: only the rows of one chunk are ever gathered).  Every result is
float64.  The work is chunked over images and rows so that the float64 temporaries of one call stay near 2 GB.

The acceptance bound
--------------------
``S`` is the sum of the magnitudes of the very terms the result sums, e.g. for the apply

    S[b,0,y,x] = sum_img sum_fy |v_fy| sum_fx |h_fx| |pixel(y+fy, x+fx)|

An fp32 evaluation that spends ``m`` rounded operations on the path of any one term -- in any order, as a tree or a chain, fused
or not -- errs by at most gamma_m * sum|terms|, gamma_m = m u / (1 - m u), u = 2^-24 (Higham, Accuracy and Stability of Numerical
Algorithms, 3.1 and 3.4).  ``assert_within_rounding`` checks  |got - ref| <= n * 2^-24 * S + 2^-100  at every element, with n >= m
derived below and never tuned (2^-100 covers flushed fp32 subnormals: 2601 terms below 2^-126 each; gamma_m / (m u) < 1.00001 for
these m, which the margin between m and n absorbs).

* Fused apply and forward op, per output: 51 fma along x, 51 fma along y, for the apply the channel mean ``(o + o) + o`` (2), the
  add of the other image's parked sum (1), the multiply by float32(1/3) (1) and that constant's own rounding (1): at most 107.
  **N_APPLY = 110.**  The forward op alone has 102 and uses the same n.
* Gradients, for each of gradVertical and gradHorizontal: 3 x 51 products and sums over the channels and the other axis' taps, then
  the remaining factor and the final sums: at most 157.  **N_GRAD = 161.**  The gray forms sum the three gradient channels first
  (2 more additions inside the same count) and have the same S, since |g0 + g1 + g2| <= |g0| + |g1| + |g2|.

The reference's own float64 error (about 2600 * 2^-53 * S) is 2^-18 of one unit of the bound.
"""
import torch
import torch.nn.functional as F

K = 51
PAD = K // 2
N_APPLY = 110
N_GRAD = 161
U = 2.0 ** -24
ABS_SLACK = 2.0 ** -100
_CHUNK_PIXELS = 1 << 21          # output pixels per chunk: two coefficient chunks in float64 are 2 * 51 * 8 B * 2^21 = 1.7 GB


def _chunks(B, H, W, budget=None):
    """(b0, b1, y0, y1): whole images while several fit the pixel budget, otherwise one image's rows at a time."""
    budget = budget or _CHUNK_PIXELS
    if H * W <= budget:
        nb = max(1, budget // max(H * W, 1))
        for b0 in range(0, B, nb):
            yield b0, min(B, b0 + nb), 0, H
        return
    rows = max(1, budget // W)
    for b in range(B):
        for y0 in range(0, H, rows):
            yield b, b + 1, y0, min(H, y0 + rows)


def _coef64(k, b0, b1, y0, y1, W):
    """Rows y0:y1 of images b0:b1 of a coefficient tensor as float64 [nb,51,rows,W] (NCHW, or the permuted view of a blocked tensor)."""
    c = k[b0:b1, :, y0:y1].to(torch.float64)
    if c.dim() == 5:
        c = c.reshape(b1 - b0, K, y1 - y0, -1)[..., :W]
    assert c.shape == (b1 - b0, K, y1 - y0, W), (tuple(k.shape), tuple(c.shape))
    return c


def _sep_chunk(p, v, h, rows, W):
    """p: padded rows [nb,C,rows+50,W+50]; v, h: [nb,51,rows,W], all float64.  Returns (sum, sum of magnitudes)."""
    pa, va, ha = p.abs(), v.abs(), h.abs()
    acc = p.new_zeros(p.shape[0], p.shape[1], rows, W)
    acc_a = torch.zeros_like(acc)
    inner = torch.empty_like(acc)
    inner_a = torch.empty_like(acc)
    for fy in range(K):
        inner.zero_()
        inner_a.zero_()
        for fx in range(K):
            inner.addcmul_(h[:, fx:fx + 1], p[:, :, fy:fy + rows, fx:fx + W])
            inner_a.addcmul_(ha[:, fx:fx + 1], pa[:, :, fy:fy + rows, fx:fx + W])
        acc.addcmul_(v[:, fy:fy + 1], inner)
        acc_a.addcmul_(va[:, fy:fy + 1], inner_a)
    return acc, acc_a


def forward_ref64(inp, ver, hor):
    """out[b,c,y,x] = sum_fy ver[b,fy,y,x] sum_fx hor[b,fx,y,x] inp[b,c,y+fy,x+fx]  and the same sum over magnitudes."""
    B, C, Hp, Wp = inp.shape
    H, W = Hp - (K - 1), Wp - (K - 1)
    assert ver.shape[0] == B and ver.shape[1] == K and ver.shape[2] == H and hor.shape[:3] == ver.shape[:3]
    ref = torch.empty(B, C, H, W, dtype=torch.float64, device=inp.device)
    S = torch.empty_like(ref)
    for b0, b1, y0, y1 in _chunks(B, H, W, _CHUNK_PIXELS // max(C, 1)):
        p = inp[b0:b1, :, y0:y1 + K - 1].to(torch.float64)
        v, h = _coef64(ver, b0, b1, y0, y1, W), _coef64(hor, b0, b1, y0, y1, W)
        ref[b0:b1, :, y0:y1], S[b0:b1, :, y0:y1] = _sep_chunk(p, v, h, y1 - y0, W)
    return ref, S


def apply_ref64(g1, g2, k1v, k1h, k2v, k2h):
    """mean_c(sepconv(pad(i2), k2v, k2h) + sepconv(pad(i1), k1v, k1h)) on frames whose three channels are the plane g: the mean of
    three equal values is the value, so ref = sep(g2) + sep(g1); S sums the magnitudes of the terms of both images."""
    B, C, H, W = g1.shape
    assert C == 1 and g2.shape == g1.shape
    ref = torch.zeros(B, 1, H, W, dtype=torch.float64, device=g1.device)
    S = torch.zeros_like(ref)
    for g, kv, kh in ((g2, k2v, k2h), (g1, k1v, k1h)):
        for b0, b1, y0, y1 in _chunks(B, H, W):
            pad = F.pad(g[b0:b1].to(torch.float64), (PAD, PAD, PAD, PAD), mode="replicate")
            v, h = _coef64(kv, b0, b1, y0, y1, W), _coef64(kh, b0, b1, y0, y1, W)
            r, s = _sep_chunk(pad[:, :, y0:y1 + K - 1], v, h, y1 - y0, W)
            ref[b0:b1, :, y0:y1] += r
            S[b0:b1, :, y0:y1] += s
            del pad, v, h, r, s
    return ref, S


def backward_ref64(grad, inp, ver, hor):
    """gv[b,fy,y,x] = sum_c grad[b,c,y,x] sum_fx hor[b,fx,y,x] inp[b,c,y+fy,x+fx]
    gh[b,fx,y,x] = sum_c grad[b,c,y,x] sum_fy ver[b,fy,y,x] inp[b,c,y+fy,x+fx]      and the same sums over magnitudes."""
    B, C, Hp, Wp = inp.shape
    H, W = Hp - (K - 1), Wp - (K - 1)
    assert grad.shape == (B, C, H, W) and ver.shape[:3] == (B, K, H) and hor.shape[:3] == (B, K, H)
    dev = inp.device
    gv = torch.empty(B, K, H, W, dtype=torch.float64, device=dev)
    gh, S_gv, S_gh = torch.empty_like(gv), torch.empty_like(gv), torch.empty_like(gv)
    for b0, b1, y0, y1 in _chunks(B, H, W, _CHUNK_PIXELS // 4):          # eight 51-plane float64 tensors per chunk
        rows = y1 - y0
        p = inp[b0:b1, :, y0:y1 + K - 1].to(torch.float64)
        pa = p.abs()
        g = grad[b0:b1, :, y0:y1].to(torch.float64)
        ga = g.abs()
        v, h = _coef64(ver, b0, b1, y0, y1, W), _coef64(hor, b0, b1, y0, y1, W)
        va, ha = v.abs(), h.abs()
        cgv = torch.zeros(b1 - b0, K, rows, W, dtype=torch.float64, device=dev)
        cgh, cav, cah = torch.zeros_like(cgv), torch.zeros_like(cgv), torch.zeros_like(cgv)
        for fy in range(K):
            for fx in range(K):
                win = p[:, :, fy:fy + rows, fx:fx + W]
                gp = (g * win).sum(dim=1)                                        # sum over channels: [nb,rows,W]
                gpa = (ga * pa[:, :, fy:fy + rows, fx:fx + W]).sum(dim=1)
                cgv[:, fy].addcmul_(h[:, fx], gp)
                cgh[:, fx].addcmul_(v[:, fy], gp)
                cav[:, fy].addcmul_(ha[:, fx], gpa)
                cah[:, fx].addcmul_(va[:, fy], gpa)
        gv[b0:b1, :, y0:y1], gh[b0:b1, :, y0:y1] = cgv, cgh
        S_gv[b0:b1, :, y0:y1], S_gh[b0:b1, :, y0:y1] = cav, cah
    return gv, gh, S_gv, S_gh


def rounding_report(got, ref, S, n):
    """Where ``got`` leaves  |got - ref| <= n * 2^-24 * S + 2^-100  (a NaN or Inf in ``got`` counts as leaving it).
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
    """Every element of ``got`` [B,*,H,W] within the derived rounding bound of ``ref``; returns the worst err / (2^-24 S).  The
    failure message carries the position of the first bad element in the terms a kernel's lanes, tiles and rows are laid out in."""
    rep = rounding_report(got, ref, S, n)
    if rep["bad"]:
        b, c, y, x = rep["first"]
        H = got.shape[2]
        raise AssertionError(
            "%s: %d of %d elements outside %d * 2^-24 * S (%d not finite); worst err / (2^-24 S) = %.4g; first bad element "
            "[b=%d, c=%d, y=%d, x=%d] at ratio %.4g: (x mod 4, x mod 64, y mod 64, y, H - y, b) = (%d, %d, %d, %d, %d, %d)"
            % (what, rep["bad"], got.numel(), n, rep["nonfinite"], rep["worst"], b, c, y, x, rep["first_ratio"],
               x % 4, x % 64, y % 64, y, H - y, b))
    return rep["worst"]
