"""float64 restatements of the single-scale SSIM criterion (SSIMLoss of sff_scripts_interp/loss/loss_ssim.py:74-146) for
tests/test_ssim_loss_cpu.py and tests/test_ssim_loss_gpu.py, and the cases they share with tests/golden/make_ssim_loss_golden.py.
Plain torch on whatever device the images live on; nothing here is imported by the package.

* ``ref64``     the reference's formulation -- its own fp32 2-D window widened to float64, grouped convolutions with padding 5 -- under
                autograd: the yardstick of the GPU checks.
* ``manual64``  the formulas the kernels implement (csrc/ssim_loss_kernels.hip): separable taps, the map's derivatives (a, b, c), the
                second blur (the blur is its own adjoint) and the scale -grad / N -- no autograd.  ``mutant`` breaks one of them.
* ``make_case`` the images: ms_ssim_ref64.make_pair's recipe (already inside [0, 1]), B C planes of it, rounded to multiples of 1 / 4096
                (exact in fp32: 12-bit images, which is what keeps the fixture below ms_ssim.npz's size); the last case is two constants.

The value is the LOSS, 1 - mean(ssim map): a scalar, or [B] with size_average=False.  Gradients are those of ``(grad_value * value).sum()``
with grad_value = ones unless given (a scalar, or [B]).
"""
import numpy as np
import torch
import torch.nn.functional as F

import ms_ssim_ref64 as M

# (B, C, H, W), size_average
CASES = (((1, 1, 5, 7), True), ((1, 1, 11, 11), True), ((2, 1, 33, 31), True), ((2, 3, 45, 70), True), ((1, 1, 96, 80), True),
         ((3, 1, 20, 40), False), ((1, 1, 16, 16), True))
CONSTANT_CASE = len(CASES) - 1            # pred = 0.05, target = 0.1 everywhere: zero variances away from the border, a finite map
GRID = 4096.0
MUTANTS = ("shrunk_window", "max_val", "dropped_x_blur_b", "batch_mean", "swapped_images")
C1, C2 = 0.01 ** 2, 0.03 ** 2


def case_seed(index):
    return 9300 + index


def make_case(index):
    """(pred, target) float32 numpy [B,C,H,W] of case ``index``."""
    (B, C, H, W), _ = CASES[index]
    if index == CONSTANT_CASE:
        return np.full((B, C, H, W), 0.05, np.float32), np.full((B, C, H, W), 0.1, np.float32)
    p, t = M.make_pair(B * C, H, W, case_seed(index))
    on_grid = lambda a: (np.round(a.astype(np.float64) * GRID) / GRID).astype(np.float32).reshape(B, C, H, W)  # noqa: E731
    return on_grid(p), on_grid(t)


def taps32():
    return M.taps32(11)                    # sigma = 1.5 * 11 / 11


def window32(channel):
    return M.window32(11).expand(channel, 1, 11, 11).contiguous()


def _weights(value, grad_value):
    if grad_value is None:
        return torch.ones_like(value)
    return grad_value.detach().to(device=value.device, dtype=torch.float64).expand_as(value)


def ref64(img1, img2, size_average=True, want_grad2=False, grad_value=None):
    """-> value (float64: 0-d, or [B]), d / d img1 (and d / d img2)."""
    a = img1.detach().to(torch.float64).requires_grad_(True)
    b = img2.detach().to(torch.float64).requires_grad_(want_grad2)
    C = a.shape[1]
    win = window32(C).to(device=a.device, dtype=torch.float64)
    blur = lambda t: F.conv2d(t, win, padding=5, groups=C)  # noqa: E731
    mu1, mu2 = blur(a), blur(b)
    m11, m22, m12 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s11, s22, s12 = blur(a * a) - m11, blur(b * b) - m22, blur(a * b) - m12
    ssim_map = ((2 * m12 + C1) * (2 * s12 + C2)) / ((m11 + m22 + C1) * (s11 + s22 + C2))
    value = 1 - (ssim_map.mean() if size_average else ssim_map.mean(1).mean(1).mean(1))
    grads = torch.autograd.grad((value * _weights(value, grad_value)).sum(), [a, b] if want_grad2 else [a])
    return (value.detach(), grads[0]) + ((grads[1],) if want_grad2 else ())


def _blur(t, g, p):
    """Separable blur of [B,C,H,W] with taps g and zero padding p, every plane alike."""
    B, C, H, W = t.shape
    return M._blur(t.reshape(B * C, 1, H, W), g, p).reshape(B, C, H + 2 * p - g.numel() + 1, W + 2 * p - g.numel() + 1)


def manual64(img1, img2, size_average=True, grad_value=None, mutant=None):
    """-> value, d / d img1 by the kernels' formulas in float64.  mutant: one of MUTANTS, a deliberately wrong variant."""
    assert mutant is None or mutant in MUTANTS
    x, y = img1.detach().to(torch.float64), img2.detach().to(torch.float64)
    if mutant == "swapped_images":         # the gradient of the other image
        x, y = y, x
    B, C, H, W = x.shape
    ws = min(H, W, 11) if mutant == "shrunk_window" else 11
    g = M.taps32(ws).to(device=x.device, dtype=torch.float64) if ws != 11 else taps32().to(device=x.device, dtype=torch.float64)
    p = ws // 2
    c2 = (0.03 * 255) ** 2 if mutant == "max_val" else C2
    mu1, mu2 = _blur(x, g, p), _blur(y, g, p)
    e11, e22, e12 = _blur(x * x, g, p), _blur(y * y, g, p), _blur(x * y, g, p)
    A1, A2 = 2 * mu1 * mu2 + C1, 2 * (e12 - mu1 * mu2) + c2
    B1, B2 = mu1 ** 2 + mu2 ** 2 + C1, (e11 - mu1 ** 2) + (e22 - mu2 ** 2) + c2
    mcs, r = A2 / B2, A1 / B1
    ssim_map = r * mcs
    a = (2 * mu2 / B1 - 2 * mu1 * A1 / B1 ** 2) * mcs + r * (-2 * mu2 / B2 + 2 * mu1 * A2 / B2 ** 2)
    b = r * (-A2 / B2 ** 2)
    c = r * (2 / B2)
    if size_average:
        value = 1 - ssim_map.mean()
        n = ssim_map.numel()
    elif mutant == "batch_mean":
        value = (1 - ssim_map.mean()).expand(B).clone()
        n = ssim_map.numel()
    else:
        value = 1 - ssim_map.mean(dim=(1, 2, 3))
        n = ssim_map.numel() // B
    gv = _weights(value, grad_value).reshape(-1, 1, 1, 1)
    second = _blur(b, g, p)
    if mutant == "dropped_x_blur_b":
        second = torch.zeros_like(second)
    grad = -(gv / n) * (_blur(a, g, p) + 2 * x * second + y * _blur(c, g, p))
    return value, grad
