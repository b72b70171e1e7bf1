"""float64 restatements of the MS-SSIM criterion for tests/test_ms_ssim_cpu.py and tests/test_ms_ssim_gpu.py, and the input recipe
they share with tests/golden/make_ms_ssim_golden.py.  Plain torch on whatever device the images live on; nothing here is imported by
the package.

* ``ref64``     the reference's formulation (sff_scripts_fusion/loss/loss_ssim.py:18-72) with its own fp32 2-D window widened to
                float64, under autograd: the yardstick of the GPU checks.
* ``manual64``  the formulas the kernels implement (csrc/ssim_kernels.hip): separable taps, the map derivatives (a, b, c), the
                adjoint blur, the gather from the coarser level and the per-level coefficients -- no autograd.
* ``make_pair`` the images: smooth-ish, correlated, so that every level's mcs mean sits well inside (0, 1).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)

# [B, H, W], max_val: the fixture's cases ([B,1,H,W] images)
CASES = (((2, 32, 32), 1.0), ((1, 33, 95), 1.0), ((2, 37, 70), 1.0), ((1, 40, 44), 1.0), ((1, 48, 32), 1.0), ((3, 64, 48), 1.0),
         ((2, 32, 32), 255.0))


def _octaves(rng, B, H, W, amplitude):
    out = np.zeros((B, 1, H, W), dtype=np.float64)
    for s in (1, 2, 4, 8, 16):
        coarse = rng.uniform(-amplitude, amplitude, size=(B, 1, -(-H // s), -(-W // s)))
        out += np.repeat(np.repeat(coarse, s, axis=2), s, axis=3)[:, :, :H, :W]
    return out


def make_pair(B, H, W, seed, scale=1.0):
    """(pred, target) float32 numpy [B,1,H,W]: target = 0.5 + nearest-upsampled uniform noise at octaves 1, 2, 4, 8, 16 px of amplitude
    0.12, pred = target + the same construction at amplitude 0.06, both clamped to [0, 1] (then times ``scale``)."""
    rng = np.random.default_rng(seed)
    target = 0.5 + _octaves(rng, B, H, W, 0.12)
    pred = target + _octaves(rng, B, H, W, 0.06)
    clamp = lambda a: (np.clip(a, 0.0, 1.0) * scale).astype(np.float32)  # noqa: E731
    return clamp(pred), clamp(target)


def case_seed(index):
    return 9100 + index


def taps32(ws):
    """The window's 1-D taps as the reference forms them: double exponentials rounded to fp32, divided by their fp32 sum."""
    sigma = 1.5 * ws / 11
    g = torch.tensor([math.exp(-(k - ws // 2) ** 2 / float(2 * sigma ** 2)) for k in range(ws)], dtype=torch.float32)
    return g / g.sum()


def window32(ws):
    """... and its 2-D window, the fp32 outer product (create_window, loss_ssim.py:12-16)."""
    g = taps32(ws).unsqueeze(1)
    return g.mm(g.t()).float()[None, None]


def ref64(img1, img2, max_val=1.0, levels=5, want_grad2=False):
    """-> value (float64 scalar tensor), terms [levels, 2] = (ssim mean, mcs mean), d value / d img1 (and / d img2)."""
    a = img1.detach().to(torch.float64).requires_grad_(True)
    b = img2.detach().to(torch.float64).requires_grad_(want_grad2)
    C1, C2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    x, y = a, b
    ssims, mcss = [], []
    for _ in range(levels):
        ws = min(x.shape[2], x.shape[3], 11)
        win = window32(ws).to(device=x.device, dtype=torch.float64)
        blur = lambda t: F.conv2d(t, win, padding=ws // 2)  # noqa: E731
        mu1, mu2 = blur(x), blur(y)
        m11, m22, m12 = mu1.pow(2), mu2.pow(2), mu1 * mu2
        s11, s22, s12 = blur(x * x) - m11, blur(y * y) - m22, blur(x * y) - m12
        V1, V2 = 2.0 * s12 + C2, s11 + s22 + C2
        ssims.append((((2 * m12 + C1) * V1) / ((m11 + m22 + C1) * V2)).mean())
        mcss.append((V1 / V2).mean())
        x, y = F.avg_pool2d(x, 2, 2), F.avg_pool2d(y, 2, 2)
    w = torch.tensor(WEIGHTS, dtype=torch.float32).to(device=a.device, dtype=torch.float64)
    ssim_t, mcs_t = torch.stack(ssims), torch.stack(mcss)
    value = torch.prod(mcs_t[:levels - 1] ** w[:levels - 1]) * ssim_t[levels - 1] ** w[levels - 1]
    grads = torch.autograd.grad(value, [a, b] if want_grad2 else [a])
    terms = torch.stack((ssim_t, mcs_t), 1).detach()
    return (value.detach(), terms, grads[0]) + ((grads[1],) if want_grad2 else ())


def _blur(t, g, p):
    ws = g.numel()
    t = F.conv2d(t, g.view(1, 1, 1, ws), padding=(0, p))
    return F.conv2d(t, g.view(1, 1, ws, 1), padding=(p, 0))


def _blur_adjoint_axis(f, g, p, n, axis):
    """out[j] = sum_k g[k] f[j - k + p] along ``axis``, j in [0, n), f zero outside its extent."""
    ws = g.numel()
    pad = [0, 0, 0, 0]
    pad[0 if axis == 3 else 2] = pad[1 if axis == 3 else 3] = ws
    fp = F.pad(f, pad)
    out = 0
    for k in range(ws):
        start = ws + p - k
        out = out + g[k] * (fp[:, :, :, start:start + n] if axis == 3 else fp[:, :, start:start + n, :])
    return out


def manual64(img1, img2, max_val=1.0, levels=5):
    """-> value, terms [levels, 2], d value / d img1 by the kernels' formulas in float64."""
    C1, C2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    x, y = img1.detach().to(torch.float64), img2.detach().to(torch.float64)
    pyr, derivs, terms, counts = [], [], [], []
    for i in range(levels):
        h, w = x.shape[2], x.shape[3]
        ws = min(h, w, 11)
        p = ws // 2
        g = taps32(ws).to(device=x.device, dtype=torch.float64)
        mu1, mu2 = _blur(x, g, p), _blur(y, g, p)
        e11, e22, e12 = _blur(x * x, g, p), _blur(y * y, g, p), _blur(x * y, g, p)
        assert mu1.shape[2] == h + 2 * p - ws + 1 and mu1.shape[3] == w + 2 * p - ws + 1
        A1, A2 = 2 * mu1 * mu2 + C1, 2 * (e12 - mu1 * mu2) + C2
        B1, B2 = mu1 ** 2 + mu2 ** 2 + C1, (e11 - mu1 ** 2) + (e22 - mu2 ** 2) + C2
        mcs, r = A2 / B2, A1 / B1
        a, b, c = -2 * mu2 / B2 + 2 * mu1 * A2 / B2 ** 2, -A2 / B2 ** 2, 2 / B2
        if i == levels - 1:
            a, b, c = (2 * mu2 / B1 - 2 * mu1 * A1 / B1 ** 2) * mcs + r * a, r * b, r * c
        terms.append(((r * mcs).mean(), mcs.mean()))
        counts.append(mcs.numel())
        pyr.append((x, y, g, p))
        derivs.append((a, b, c))
        x, y = F.avg_pool2d(x, 2, 2), F.avg_pool2d(y, 2, 2)
    used = [terms[i][1] if i < levels - 1 else terms[i][0] for i in range(levels)]
    wts = [float(np.float32(v)) for v in WEIGHTS]
    value = 1.0
    for i in range(levels):
        value = value * used[i] ** wts[i]
    grad = None
    for i in reversed(range(levels)):
        x, y, g, p = pyr[i]
        h, w = x.shape[2], x.shape[3]
        adj = lambda f: _blur_adjoint_axis(_blur_adjoint_axis(f, g, p, w, 3), g, p, h, 2)  # noqa: E731
        a, b, c = derivs[i]
        coef = wts[i] * value / (used[i] * counts[i])
        here = coef * (adj(a) + 2 * x * adj(b) + y * adj(c))
        if grad is not None:
            up = 0.25 * grad.repeat_interleave(2, 2).repeat_interleave(2, 3)
            here[:, :, :up.shape[2], :up.shape[3]] += up
        grad = here
    t = torch.stack([torch.stack(tt) for tt in terms])
    return value, t, grad
