"""``MS_SSIM`` -- the reference's multi-scale SSIM criterion on MI355X.

Mirrors ``sff_scripts_fusion/loss/loss_ssim.py:18-72`` of the reference: the same import path (``from loss.loss_ssim import MS_SSIM``),
constructor ``MS_SSIM(size_average=True, max_val=255)`` and ``forward(img1, img2) -> scalar`` over five pyramid levels.  The
arithmetic is native (``include/sstem_loss.h``, ``csrc/ssim_kernels.hip``): one launch per level for the value, one per level for the
gradient of each image that requires one, every sum in a fixed order -- torch's formulation is five 11 x 11 convolutions and about
twenty pointwise launches per level, twice over for the backward.

* GPU tensors only: CPU tensors raise ``NotImplementedError``, like every native op of the package.
* ``[B,1,H,W]`` float32 only (the reference's window has one channel: other channel counts fail there too, in ``F.conv2d``),
  ``min(H, W) >= 32`` for the five levels (the reference fails below that in its trailing ``avg_pool2d``).
* One instance belongs to ONE stream: it owns the workspace its launches reduce through and leave the pyramids in (it grows when a
  larger shape arrives, outside graph capture), and two calls in flight on two streams would share it.  The backward pass reads what
  the instance's LAST forward left there: run ``loss.backward()`` before the same instance's next forward.

``ms_ssim_torch`` is the same function as plain torch operations under autograd -- what a user could run without the native
library; ``SSTEM_NATIVE_SSIM=0`` makes ``steps.FusionStep(loss="ssim")`` use it (A/B runs, like ``SSTEM_NATIVE_L1``).

``SSIMLoss`` / ``ssim`` / ``create_window`` / ``gaussian`` -- the single-scale criterion of the interpolation loop, at the same import
path (``from loss.loss_ssim import SSIMLoss``: sff_scripts_interp/main_ms.py:27; sff_scripts_interp/loss/loss_ssim.py:74-146).
``SSIMLoss(window_size=11, size_average=True)(img1, img2)`` is ``1 - mean(ssim map)`` (one scalar, or ``[B]`` with
``size_average=False``) for ``[B,C,H,W]`` float32 GPU tensors of any channel count and any extent (the window stays 11 taps, sigma 1.5,
zero padding 5; no ``max_val``); ``ssim`` is the similarity itself.  One launch for the value, one for the gradient of each image that
requires one (``include/sstem_loss.h``, ``csrc/ssim_loss_kernels.hip``).  Only ``window_size=11`` is built: another raises
``NotImplementedError``.  ``ssim_loss_torch`` is the plain-torch formulation (``SSTEM_NATIVE_SSIM=0`` makes
``steps.IFNetStep(loss="ssim")`` use it).
"""
import math

import torch
import torch.nn.functional as F

import sstem_native

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


class _Workspace:
    """The launches' workspace for one caller: zero when created (the library leaves it clean after every call)."""

    def __init__(self):
        self.lib = sstem_native.load_library()
        self.buf = None

    def get(self, B, H, W, levels, device):
        need = int(self.lib.sstem_ms_ssim_workspace_floats(B, H, W, levels))
        if need <= 0:
            # the forward entry says why
            return self.buf if self.buf is not None else torch.zeros(64, dtype=torch.float32, device=device)
        if self.buf is None or self.buf.numel() < need or self.buf.device != device:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("MS_SSIM: the workspace has to grow for shape %r -- run this shape once before capturing" % ((B, 1, H, W),))
            self.buf = torch.zeros(need, dtype=torch.float32, device=device)
        return self.buf


def _check_images(img1, img2):
    if not (img1.is_cuda and img2.is_cuda):
        raise NotImplementedError("MS_SSIM is GPU-only")
    if img1.dtype != torch.float32 or img2.dtype != torch.float32:
        raise TypeError("MS_SSIM: float32 images")
    if img1.dim() != 4 or img1.shape[1] != 1 or img1.shape != img2.shape:
        raise ValueError("MS_SSIM: two [B,1,H,W] images of one shape, got %r and %r" % (tuple(img1.shape), tuple(img2.shape)))


def _forward(lib, wsp, a, b, max_val, levels, terms=None):
    B, _, H, W = a.shape
    ws = wsp.get(B, H, W, levels, a.device)
    value = torch.empty((), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        rc = lib.sstem_ms_ssim_forward_f32(a.data_ptr(), b.data_ptr(), B, H, W, levels, max_val, value.data_ptr(),
                                           terms.data_ptr() if terms is not None else None, ws.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream)
    sstem_native.check(rc, "sstem_ms_ssim_forward_f32")
    return value, ws


def _backward(lib, ws, first, second, max_val, levels, grad_value):
    B, _, H, W = first.shape
    grad = torch.empty_like(first)
    with torch.cuda.device(first.device):
        rc = lib.sstem_ms_ssim_backward_f32(first.data_ptr(), second.data_ptr(), B, H, W, levels, max_val,
                                            grad_value.data_ptr() if grad_value is not None else None, grad.data_ptr(), ws.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream)
    sstem_native.check(rc, "sstem_ms_ssim_backward_f32")
    return grad


class _MSSSIMFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2, wsp, max_val, levels):
        a, b = img1.contiguous(), img2.contiguous()
        value, ws = _forward(wsp.lib, wsp, a, b, max_val, levels)
        ctx.save_for_backward(a, b)
        ctx.ws, ctx.lib, ctx.max_val, ctx.levels = ws, wsp.lib, max_val, levels
        return value

    @staticmethod
    def backward(ctx, grad_value):
        a, b = ctx.saved_tensors
        if not grad_value.is_cuda:
            raise NotImplementedError("MS_SSIM is GPU-only")
        gv = grad_value.to(torch.float32).contiguous()
        g1 = _backward(ctx.lib, ctx.ws, a, b, ctx.max_val, ctx.levels, gv) if ctx.needs_input_grad[0] else None
        # symmetric function: the second image's gradient is the same launch with the operands exchanged
        g2 = _backward(ctx.lib, ctx.ws, b, a, ctx.max_val, ctx.levels, gv) if ctx.needs_input_grad[1] else None
        return g1, g2, None, None, None


class MS_SSIM(torch.nn.Module):
    def __init__(self, size_average=True, max_val=255):
        super(MS_SSIM, self).__init__()
        self.size_average = size_average
        self.channel = 1
        self.max_val = max_val
        self._wsp = _Workspace()

    def ms_ssim(self, img1, img2, levels=5):
        _check_images(img1, img2)
        return _MSSSIMFunction.apply(img1, img2, self._wsp, float(self.max_val), int(levels))

    def level_terms(self, img1, img2, levels=5):
        """``(value, terms[levels, 2])``: the value and every level's (ssim mean, mcs mean) -- no gradient (tests, diagnostics)."""
        _check_images(img1, img2)
        terms = torch.empty(levels, 2, dtype=torch.float32, device=img1.device)
        value, _ = _forward(self._wsp.lib, self._wsp, img1.detach().contiguous(), img2.detach().contiguous(), float(self.max_val),
                            int(levels), terms)
        return value, terms

    def forward(self, img1, img2):
        return self.ms_ssim(img1, img2)


def _window(ws, dtype, device):
    sigma = 1.5 * ws / 11
    g = torch.tensor([math.exp(-(k - ws // 2) ** 2 / float(2 * sigma ** 2)) for k in range(ws)], dtype=torch.float32)
    g = g / g.sum()
    return torch.outer(g, g).to(device=device, dtype=dtype)[None, None]


def ms_ssim_torch(img1, img2, max_val=1.0, levels=5):
    """The criterion as plain torch operations (2-D window convolutions, pointwise maps, ``avg_pool2d``) under autograd: any device,
    any float dtype.  The A/B partner of the native path, not a fallback: nothing selects it unless asked."""
    C1, C2 = (0.01 * max_val) ** 2, (0.03 * max_val) ** 2
    terms = []
    for i in range(levels):
        ws = min(img1.shape[2], img1.shape[3], 11)
        win = _window(ws, img1.dtype, img1.device)
        blur = lambda t: F.conv2d(t, win, padding=ws // 2)  # noqa: E731
        mu1, mu2 = blur(img1), blur(img2)
        m11, m22, m12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
        A2 = 2.0 * (blur(img1 * img2) - m12) + C2
        B2 = (blur(img1 * img1) - m11) + (blur(img2 * img2) - m22) + C2
        if i == levels - 1:
            terms.append((((2 * m12 + C1) * A2) / ((m11 + m22 + C1) * B2)).mean())
        else:
            terms.append((A2 / B2).mean())
        img1, img2 = F.avg_pool2d(img1, 2, 2), F.avg_pool2d(img2, 2, 2)
    w = torch.tensor(WEIGHTS[:levels], dtype=torch.float32, device=img1.device).to(img1.dtype)
    return torch.prod(torch.stack(terms) ** w)


# ---- single-scale SSIM: SSIMLoss / ssim of the interpolation loop ------------------------------------------------------------------
def gaussian(window_size, sigma):
    """The window's 1-D taps, fp32, normalised by their fp32 sum."""
    half, two_var = window_size // 2, 2.0 * sigma * sigma
    g = torch.tensor([math.exp(-((k - half) ** 2) / two_var) for k in range(window_size)], dtype=torch.float32)
    return g / g.sum()


def create_window(window_size, channel):
    """``[channel, 1, window_size, window_size]``: the fp32 outer product of the taps at sigma 1.5, one copy per channel."""
    g = gaussian(window_size, 1.5)
    return torch.outer(g, g)[None, None].expand(channel, 1, window_size, window_size).contiguous()


class _SSIMLossWorkspace:
    """The single-scale launches' workspace for one caller: zero when created (the library leaves it clean after every call)."""

    def __init__(self):
        self.lib = sstem_native.load_library()
        self.buf = None

    def get(self, shape, device):
        need = max(16, int(self.lib.sstem_ssim_loss_workspace_floats(*shape)))       # an empty or refused shape: the entry says why
        if self.buf is None or self.buf.numel() < need or self.buf.device != device:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("SSIMLoss: the workspace has to grow for shape %r -- run this shape once before capturing" % (tuple(shape),))
            self.buf = torch.zeros(need, dtype=torch.float32, device=device)
        return self.buf


def _check_ssim_loss_images(img1, img2, window_size=11):
    if window_size != 11:
        raise NotImplementedError("SSIMLoss: only window_size=11 is built (got %r)" % (window_size,))
    if not (img1.is_cuda and img2.is_cuda):
        raise NotImplementedError("SSIMLoss is GPU-only")
    if img1.dtype != torch.float32 or img2.dtype != torch.float32:
        raise TypeError("SSIMLoss: float32 images")
    if img1.dim() != 4 or img1.shape != img2.shape:
        raise ValueError("SSIMLoss: two [B,C,H,W] images of one shape, got %r and %r" % (tuple(img1.shape), tuple(img2.shape)))


def _ssim_loss_forward(wsp, a, b, per_sample):
    B = a.shape[0]
    ws = wsp.get(a.shape, a.device)
    value = torch.empty((B,) if per_sample else (), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        rc = wsp.lib.sstem_ssim_loss_forward_f32(a.data_ptr(), b.data_ptr(), *a.shape, 1 if per_sample else 0, value.data_ptr(),
                                                 ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    sstem_native.check(rc, "sstem_ssim_loss_forward_f32")
    return value, ws


def _ssim_loss_backward(lib, ws, first, second, per_sample, grad_value):
    grad = torch.empty_like(first)
    with torch.cuda.device(first.device):
        rc = lib.sstem_ssim_loss_backward_f32(first.data_ptr(), second.data_ptr(), *first.shape, 1 if per_sample else 0,
                                              grad_value.data_ptr() if grad_value is not None else None, grad.data_ptr(), ws.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream)
    sstem_native.check(rc, "sstem_ssim_loss_backward_f32")
    return grad


class _SSIMLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2, wsp, per_sample):
        a, b = img1.contiguous(), img2.contiguous()
        value, ws = _ssim_loss_forward(wsp, a, b, per_sample)
        ctx.save_for_backward(a, b)
        ctx.ws, ctx.lib, ctx.per_sample = ws, wsp.lib, per_sample
        return value

    @staticmethod
    def backward(ctx, grad_value):
        a, b = ctx.saved_tensors
        if not grad_value.is_cuda:
            raise NotImplementedError("SSIMLoss is GPU-only")
        gv = grad_value.to(torch.float32).contiguous()
        g1 = _ssim_loss_backward(ctx.lib, ctx.ws, a, b, ctx.per_sample, gv) if ctx.needs_input_grad[0] else None
        # symmetric function: the second image's gradient is the same launch with the operands exchanged
        g2 = _ssim_loss_backward(ctx.lib, ctx.ws, b, a, ctx.per_sample, gv) if ctx.needs_input_grad[1] else None
        return g1, g2, None, None


class SSIMLoss(torch.nn.Module):
    """loss = 1 - SSIM(a, b)"""

    def __init__(self, window_size=11, size_average=True):
        super(SSIMLoss, self).__init__()
        if window_size != 11:
            raise NotImplementedError("SSIMLoss: only window_size=11 is built (got %r)" % (window_size,))
        self.window_size = window_size
        self.size_average = size_average
        self.channel = 1
        self.window = create_window(window_size, self.channel)
        self._wsp = None

    def forward(self, img1, img2):
        _check_ssim_loss_images(img1, img2, self.window_size)
        if self._wsp is None:
            self._wsp = _SSIMLossWorkspace()
        self.channel = img1.shape[1]
        return _SSIMLossFunction.apply(img1, img2, self._wsp, not self.size_average)


def ssim(img1, img2, window_size=11, size_average=True):
    """The similarity itself (not the loss): ``mean(ssim map)``, or per sample with ``size_average=False``."""
    _check_ssim_loss_images(img1, img2, window_size)
    return 1 - _SSIMLossFunction.apply(img1, img2, _SSIMLossWorkspace(), not size_average)


def ssim_loss_torch(img1, img2, size_average=True):
    """``SSIMLoss`` as plain torch operations (grouped 2-D window convolutions, pointwise maps) under autograd: any device, any float
    dtype.  The A/B partner of the native path, not a fallback: nothing selects it unless asked."""
    C = img1.shape[1]
    win = create_window(11, C).to(device=img1.device, dtype=img1.dtype)
    blur = lambda t: F.conv2d(t, win, padding=5, groups=C)  # noqa: E731
    mu1, mu2 = blur(img1), blur(img2)
    m11, m22, m12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s11, s22, s12 = blur(img1 * img1) - m11, blur(img2 * img2) - m22, blur(img1 * img2) - m12
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ssim_map = ((2 * m12 + C1) * (2 * s12 + C2)) / ((m11 + m22 + C1) * (s11 + s22 + C2))
    return 1 - (ssim_map.mean() if size_average else ssim_map.mean(dim=(1, 2, 3)))
