"""float64 restatement of the back-warp's gradients (include/sstem_warp.h: sstem_warp_bilinear_backward_f32), in numpy.

Coordinates, indices and weights are taken in float32 exactly as csrc/warp_kernels.hip takes them (x = (flow + col) + 1, floor, the
4e18 guard, clamp to [0, W+1], weights from the CLAMPED x1 / y1, 1 - w in float32); every product and sum after that is float64.

    grad_flow[b,0] = sum_ch g (wy (Ic - Ia) + (1-wy) (Id - Ib))          grad_flow[b,1] = sum_ch g (wx (Ib - Ia) + (1-wx) (Id - Ic))
    grad_image    += wx wy g at (y0,x0), wx (1-wy) g at (y1,x0), (1-wx) wy g at (y0,x1), (1-wx) (1-wy) g at (y1,x1), border taps dropped

``ref64`` also returns, per element, what the error bounds of the tests are written in:
    S  [B,2,H,W]  sum_ch |g| (|wy| (|Ia| + |Ic|) + |1-wy| (|Ib| + |Id|)) and the y twin: the magnitude every rounding of a
                  flow-gradient element is relative to
    k  [B,C,H,W]  the number of in-plane tap contributions an image-gradient element receives, and  A = sum |w g|  over them
    out, out_abs  the forward value and sum |w| |I| over its four taps (the adjoint test's bound on the forward side)

``mutant`` selects one deliberate mistake (MUTANTS); tests/test_warp_grad_cpu.py holds each of them against the fixture.
"""
import numpy as np

MUTANTS = ("swap_dx_dy", "border_kept", "weight_sign", "no_channel_sum", "taps_b_c_exchanged", "trunc_for_floor")
F1 = np.float32(1.0)


def taps(flow, mutant=None):
    """flow [B,2,H,W] float32 -> x0, x1, y0, y1 (int64, padded-plane indices in [0, W+1] / [0, H+1]) and wx, wy (float32), each [B,H,W]."""
    flow = np.asarray(flow, np.float32)
    B, _, H, W = flow.shape
    col = np.arange(W, dtype=np.float32)[None, None, :]
    row = np.arange(H, dtype=np.float32)[None, :, None]
    x = ((flow[:, 0] + col).astype(np.float32) + F1).astype(np.float32)
    y = ((flow[:, 1] + row).astype(np.float32) + F1).astype(np.float32)
    rnd = np.trunc if mutant == "trunc_for_floor" else np.floor
    lim = np.float32(4.0e18)
    x0 = np.clip(rnd(x), -lim, lim).astype(np.int64)
    y0 = np.clip(rnd(y), -lim, lim).astype(np.int64)
    x1, y1 = x0 + 1, y0 + 1
    x0, x1 = np.clip(x0, 0, W + 1), np.clip(x1, 0, W + 1)
    y0, y1 = np.clip(y0, 0, H + 1), np.clip(y1, 0, H + 1)
    wx = (x1.astype(np.float32) - x).astype(np.float32)
    wy = (y1.astype(np.float32) - y).astype(np.float32)
    return x0, x1, y0, y1, wx, wy


def ref64(image, flow, g, mutant=None):
    assert mutant is None or mutant in MUTANTS
    image, flow, g = (np.asarray(a, np.float32) for a in (image, flow, g))
    B, C, H, W = image.shape
    assert flow.shape == (B, 2, H, W) and g.shape == (B, C, H, W)
    x0, x1, y0, y1, wx, wy = taps(flow, mutant)
    ux, uy = (F1 - wx).astype(np.float32), (F1 - wy).astype(np.float32)          # exact for in-plane samples
    wx, wy, ux, uy = (a.astype(np.float64)[:, None] for a in (wx, wy, ux, uy))    # [B,1,H,W]
    g64 = g.astype(np.float64)

    P = np.zeros((B, C, H + 2, W + 2), np.float64)
    P[:, :, 1:-1, 1:-1] = image
    if mutant == "border_kept":                                                  # the border repeats the edge instead of being zero
        P = np.pad(image.astype(np.float64), ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge")
    bi = np.arange(B)[:, None, None, None]
    ci = np.arange(C)[None, :, None, None]
    Y0, Y1, X0, X1 = (a[:, None] for a in (y0, y1, x0, x1))
    Ia, Ib, Ic, Id = P[bi, ci, Y0, X0], P[bi, ci, Y1, X0], P[bi, ci, Y0, X1], P[bi, ci, Y1, X1]

    tx = wy * (Ic - Ia) + uy * (Id - Ib)
    ty = wx * (Ib - Ia) + ux * (Id - Ic)
    sx = np.abs(wy) * (np.abs(Ia) + np.abs(Ic)) + np.abs(uy) * (np.abs(Ib) + np.abs(Id))
    sy = np.abs(wx) * (np.abs(Ia) + np.abs(Ib)) + np.abs(ux) * (np.abs(Ic) + np.abs(Id))
    if mutant == "weight_sign":
        tx, ty = -tx, -ty
    chans = slice(0, 1) if mutant == "no_channel_sum" else slice(None)
    gfx, gfy = (g64 * tx)[:, chans].sum(1), (g64 * ty)[:, chans].sum(1)
    if mutant == "swap_dx_dy":
        gfx, gfy = gfy, gfx
    grad_flow = np.stack([gfx, gfy], 1)
    S = np.stack([(np.abs(g64) * sx).sum(1), (np.abs(g64) * sy).sum(1)], 1)

    wa, wb, wc, wd = wx * wy, wx * uy, ux * wy, ux * uy
    out = wa * Ia + wb * Ib + wc * Ic + wd * Id
    out_abs = np.abs(wa * Ia) + np.abs(wb * Ib) + np.abs(wc * Ic) + np.abs(wd * Id)
    if mutant == "taps_b_c_exchanged":
        wb, wc = wc, wb
    Hp, Wp = H + 2, W + 2
    n = B * C * Hp * Wp
    gi, k, A = np.zeros(n), np.zeros(n, np.int64), np.zeros(n)
    base = (bi * C + ci) * Hp
    for w, Y, X in ((wa, Y0, X0), (wb, Y1, X0), (wc, Y0, X1), (wd, Y1, X1)):
        inside = np.broadcast_to((Y >= 1) & (Y <= H) & (X >= 1) & (X <= W), (B, C, H, W)).ravel()
        if mutant == "border_kept":
            Y, X, inside = np.clip(Y, 1, H), np.clip(X, 1, W), np.ones(B * C * H * W, bool)
        idx = np.broadcast_to((base + Y) * Wp + X, (B, C, H, W)).ravel()[inside]
        v = (w * g64).ravel()[inside]
        gi += np.bincount(idx, weights=v, minlength=n)
        A += np.bincount(idx, weights=np.abs(v), minlength=n)
        k += np.bincount(idx, minlength=n)
    crop = lambda a: a.reshape(B, C, Hp, Wp)[:, :, 1:-1, 1:-1].copy()        # noqa: E731
    return {"grad_flow": grad_flow, "grad_image": crop(gi), "S": S, "k": crop(k), "A": crop(A), "out": out, "out_abs": out_abs}


U = 2.0 ** -24          # unit roundoff of float32


def flow_bound(r, n):
    """n roundings, each relative to S."""
    return n * U * r["S"]


def image_bound(r, extra, absolute=0.0):
    """(k + extra) roundings relative to A, plus ``absolute`` per contribution."""
    return (r["k"] + extra) * U * r["A"] + r["k"] * absolute


def many_to_one_flow(B, H, W, ty, tx):
    """Every pixel samples the one source position (ty, tx) (0-based, multiples of 0.25 stay exact): an integer position puts weight 1
    on one pixel, a fractional one spreads every pixel's contribution over the same four addresses."""
    flow = np.zeros((B, 2, H, W), np.float32)
    flow[:, 0] = tx - np.arange(W, dtype=np.float32)[None, None, :]
    flow[:, 1] = ty - np.arange(H, dtype=np.float32)[None, :, None]
    return flow
