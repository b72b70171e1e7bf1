"""``image_warp`` -- the reference's numpy back-warp of a uint8 image (``sff_scripts_fusion/utils/image_warp.py:3-112``) on MI355X.

Same name, arguments and shape conventions: ``im`` uint8 of ndim 2, 3 or 4, ``[[num_batch], height, width, [channels]]``, ``flow``
float32 ``[[num_batch], height, width, 2]``, ``mode`` ``'nearest'`` or ``'bilinear'``; the warped uint8 image has ``im``'s shape, bit
for bit the reference's bytes, from one native launch (``include/sstem_fold.h``).  GPU tensors only -- numpy arrays and CPU tensors
raise ``NotImplementedError``; there is no CPU fallback.
"""
import torch

import sstem_native

_MODES = {"nearest": 0, "bilinear": 1}      # SSTEM_WARP_NEAREST, SSTEM_WARP_BILINEAR


def image_warp(im, flow, mode='bilinear'):
    if not isinstance(im, torch.Tensor) or not isinstance(flow, torch.Tensor) or not im.is_cuda or not flow.is_cuda:
        raise NotImplementedError("the warp kernel is GPU-only")
    if im.dtype != torch.uint8:
        raise TypeError("expected a uint8 image, got %s" % im.dtype)
    if mode not in _MODES:
        raise ValueError("mode must be 'nearest' or 'bilinear'")
    if im.dim() == 2:
        (height, width), num_batch, channels = im.shape, 1, 1
    elif im.dim() == 3:
        (height, width, channels), num_batch = im.shape, 1
    elif im.dim() == 4:
        num_batch, height, width, channels = im.shape
    else:
        raise AttributeError('The dimension of im must be 2, 3 or 4')
    assert flow.numel() == num_batch * height * width * 2 and flow.shape[-1] == 2, "flow must be [[num_batch], height, width, 2]"
    src = im.contiguous()
    fl = flow.float().contiguous()
    out = torch.empty_like(src)
    lib = sstem_native.load_library()
    with torch.cuda.device(src.device):
        rc = lib.sstem_image_warp_u8(src.data_ptr(), fl.data_ptr(), out.data_ptr(), num_batch, height, width, channels, _MODES[mode],
                                     torch.cuda.current_stream().cuda_stream)
    sstem_native.check(rc, "sstem_image_warp_u8")
    return out
