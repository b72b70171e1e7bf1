"""``compute_psnr`` / ``compute_ssim`` -- the reference's validation scores on MI355X.

Mirrors ``utils/psnr_ssim.py:7-71`` of the reference: the same import path (``from utils.psnr_ssim import compute_psnr, compute_ssim``),
names and return values.  The reference copies every prediction to the host and scores it with numpy and ``scipy.signal.convolve2d``
in float64; here the arithmetic is native (``include/sstem_score.h``, ``csrc/score_kernels.hip``): two launches score a whole batch of
image pairs, float64 throughout, every sum in a fixed order, the range branch (``np.max(img1) <= 1.0 and np.max(img2) <= 1.0``) decided
per image on the device.

* ``score_batch(a, b, clamp01=False)`` -> ``[B,3]`` float64 GPU tensor ``(mse, psnr, ssim)`` per image; nothing synchronises, so a
  validation loop reads its scores once at the end (or never leaves the device).  ``clamp01`` clamps ``a`` to [0, 1] as it is read:
  the loops' ``pred[pred>1]=1; pred[pred<0]=0`` (main_ms.py:265, main_fusion.py:330).
* ``compute_psnr(img1, img2)`` -> ``(mse, psnr)`` as Python floats, or the bare ``1000000000000`` where ``mse < 1e-10``;
  ``compute_ssim(im1, im2)`` -> float.  One image each, ``[H,W]`` or with leading singleton dimensions; they read the result back, so
  they synchronise like the reference's ``.cpu().numpy()`` does.
* GPU tensors only, float32 or uint8, H and W at least 11 (the window): a CPU tensor or a numpy array raises ``NotImplementedError``,
  like every native op of the package.  File names (the reference's ``io.imread`` branch) are not read here.
* One workspace per device and stream, owned by this module; it grows when a larger shape arrives -- outside graph capture, so run a
  shape once before capturing it.

Deviations from the reference are listed in ``include/sstem_score.h`` (a negative value in a unit-range image quantises to 0; float64
where the reference keeps float32 arrays in float32).
"""
import torch

import sstem_native

_workspaces = {}


def _workspace(lib, B, H, W, device):
    """The zeroed workspace of (device, current stream), grown to the shape at hand; the library leaves it clean after every call."""
    need = int(lib.sstem_score_workspace_bytes(B, H, W))
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(device).cuda_stream)
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < need:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("psnr_ssim: the workspace has to grow for shape %r -- run this shape once before capturing" % ((B, H, W),))
        buf = _workspaces[key] = torch.zeros(max(need, 64), dtype=torch.uint8, device=device)
    return buf


def _as_batch(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise NotImplementedError("psnr_ssim is GPU-only: %s must be a GPU tensor" % name)
    if t.dtype not in (torch.float32, torch.uint8):
        raise TypeError("psnr_ssim: %s must be float32 or uint8 (got %s)" % (name, t.dtype))
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 3:
        raise ValueError("psnr_ssim: %s must be [B,H,W] or [B,1,H,W], got %r" % (name, tuple(t.shape)))
    return t.contiguous()


def score_batch(a, b, clamp01=False):
    a, b = _as_batch(a, "a"), _as_batch(b, "b")
    if a.shape != b.shape or a.dtype != b.dtype or a.device != b.device:
        raise ValueError("psnr_ssim: two image batches of one shape, dtype and device, got %r %s and %r %s"
                         % (tuple(a.shape), a.dtype, tuple(b.shape), b.dtype))
    lib = sstem_native.load_library()
    B, H, W = a.shape
    scores = torch.empty(B, 3, dtype=torch.float64, device=a.device)
    entry = "sstem_score_images_f32" if a.dtype == torch.float32 else "sstem_score_images_u8"
    with torch.cuda.device(a.device):
        ws = _workspace(lib, B, H, W, a.device)
        rc = getattr(lib, entry)(a.data_ptr(), b.data_ptr(), B, H, W, 1 if clamp01 else 0, scores.data_ptr(), ws.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
    sstem_native.check(rc, entry)
    return scores


def _one_image(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise NotImplementedError("psnr_ssim is GPU-only: %s must be a GPU tensor" % name)
    if t.dim() < 2 or any(d != 1 for d in t.shape[:-2]):
        raise ValueError("Please input the images with 1 channel")        # the reference's words (psnr_ssim.py:47)
    return t.reshape(1, t.shape[-2], t.shape[-1])


def compute_psnr(img1, img2):
    mse, psnr, _ = score_batch(_one_image(img1, "img1"), _one_image(img2, "img2"))[0].tolist()
    if mse < 1.0e-10:
        return 1000000000000
    return mse, psnr


def compute_ssim(im1, im2):
    if isinstance(im1, torch.Tensor) and isinstance(im2, torch.Tensor) and im1.shape[-2:] != im2.shape[-2:]:
        raise ValueError("Input Imagees must have the same dimensions")      # psnr_ssim.py:45
    return score_batch(_one_image(im1, "im1"), _one_image(im2, "im2"))[0, 2].item()
