"""Float64 reference of the sepconv INPUT gradient (test infrastructure only; torch, any device).

    grad_input_ref64(grad[B,C,H,W], ver[B,taps,H,W], hor[B,taps,H,W], taps=51) -> (ref, S)      both [B,C,H+taps-1,W+taps-1], float64

    ref[b,c,Y,X] = sum_fy sum_fx grad[b,c,Y-fy,X-fx] * ver[b,fy,Y-fy,X-fx] * hor[b,fx,Y-fy,X-fx]     (source pixel inside the image)

Written as a scatter -- taps x taps shifted slice additions into a float64 plane, one per tap pair -- where the kernels gather by
target element: nothing is shared with them.  ``S`` is the same sum over the magnitudes of the terms, the scale of the acceptance
bound of tests/sepconv_ref64.py (``rounding_report``, ``assert_within_rounding``).  Coefficients may be float32 or bfloat16 (widened
exactly).

The bound's n for the kernels' order (csrc/sepconv_kernels.h): one fmaf chain over all the terms of an element, source rows then source
columns ascending, each term ``fmaf(V, fl(g * H), acc)``.  By the rule of sepconv_ref64's docstring -- the rounded operations on the path
of any one term -- the first term of a full window passes one multiply (g * H) and taps * taps fmaf: 1 + 2601 = 2602 at 51 taps.
**N_GRADINPUT = 2610**, with the same small margin the other two counts carry, derived and never tuned.  Shorter filters have shorter
chains; the one n covers them.
"""
import torch

N_GRADINPUT = 2610


def grad_input_ref64(grad, ver, hor, taps=51):
    B, C, H, W = grad.shape
    assert ver.shape == (B, taps, H, W) and hor.shape == (B, taps, H, W), (tuple(grad.shape), tuple(ver.shape), tuple(hor.shape))
    g, v, h = grad.to(torch.float64), ver.to(torch.float64), hor.to(torch.float64)
    ga, va, ha = g.abs(), v.abs(), h.abs()
    ref = torch.zeros(B, C, H + taps - 1, W + taps - 1, dtype=torch.float64, device=grad.device)
    S = torch.zeros_like(ref)
    for fy in range(taps):
        gv = g * v[:, fy:fy + 1]                        # [B,C,H,W]: every source pixel's share for target row y + fy
        gva = ga * va[:, fy:fy + 1]
        for fx in range(taps):
            ref[:, :, fy:fy + H, fx:fx + W].addcmul_(gv, h[:, fx:fx + 1])
            S[:, :, fy:fy + H, fx:fx + W].addcmul_(gva, ha[:, fx:fx + 1])
    return ref, S
