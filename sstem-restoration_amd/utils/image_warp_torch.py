"""``SpatialTransformation`` -- the reference's bilinear back-warp module on MI355X.

Same class, constructor flag and call contract as ``sff_scripts_fusion/utils/image_warp_torch.py:5-112``:
``forward(moving_image[B,C,H,W], deformation_matrix[B,H,W,2]) -> warped[B,C,H,W]`` with
``deformation_matrix[..., 0] = dx`` (columns) and ``[..., 1] = dy`` (rows).  One native gather kernel
(``include/sstem_warp.h``) instead of ~20 torch ops; no gradient is defined, as in the way the reference
uses it (the flow network is frozen and runs under ``no_grad``, ``main_fusion.py:227-235``).
GPU tensors only -- there is no CPU fallback.

``DifferentiableSpatialTransformation`` is the same module with what torch's autograd derives from the reference's
(plain-torch) module: a gradient for the moving image and one for the deformation field
(``sstem_warp_bilinear_backward_f32``; first derivatives only).
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

import sstem_native


class SpatialTransformation(nn.Module):
    def __init__(self, use_gpu=False):
        self.use_gpu = use_gpu
        super(SpatialTransformation, self).__init__()

    @torch.no_grad()
    def forward(self, moving_image, deformation_matrix):
        if not moving_image.is_cuda or not deformation_matrix.is_cuda:
            raise NotImplementedError("the warp kernel is GPU-only")
        B, C, H, W = moving_image.shape
        assert tuple(deformation_matrix.shape) == (B, H, W, 2)
        img = moving_image.float().contiguous()
        # [B,H,W,2] -> [B,2,H,W]; free when the caller made it by permuting the flow network's output
        flow = deformation_matrix.permute(0, 3, 1, 2).float().contiguous()
        out = torch.empty_like(img)
        lib = sstem_native.load_library()
        with torch.cuda.device(img.device):
            rc = lib.sstem_warp_bilinear_f32(img.data_ptr(), flow.data_ptr(), out.data_ptr(), B, C, H, W,
                                             torch.cuda.current_stream().cuda_stream)
        sstem_native.check(rc, "sstem_warp_bilinear_f32")
        return out


class _BackWarp(torch.autograd.Function):
    """The back-warp of contiguous fp32 ``img`` [B,C,H,W] by ``flow`` [B,2,H,W]; the [B,H,W,2] permute stays outside, so autograd
    carries the flow gradient back into the caller's layout."""

    @staticmethod
    def forward(ctx, img, flow):
        ctx.save_for_backward(img, flow)
        B, C, H, W = img.shape
        out = torch.empty_like(img)
        lib = sstem_native.load_library()
        with torch.cuda.device(img.device):
            rc = lib.sstem_warp_bilinear_f32(img.data_ptr(), flow.data_ptr(), out.data_ptr(), B, C, H, W,
                                             torch.cuda.current_stream().cuda_stream)
        sstem_native.check(rc, "sstem_warp_bilinear_f32")
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        img, flow = ctx.saved_tensors
        need_img, need_flow = ctx.needs_input_grad
        B, C, H, W = img.shape
        g = grad_output.float().contiguous()
        grad_img = torch.empty_like(img) if need_img else None          # the entry clears it on the stream
        grad_flow = torch.empty_like(flow) if need_flow else None
        lib = sstem_native.load_library()
        with torch.cuda.device(img.device):
            rc = lib.sstem_warp_bilinear_backward_f32(img.data_ptr() if need_flow else None, flow.data_ptr(), g.data_ptr(),
                                                      grad_flow.data_ptr() if need_flow else None,
                                                      grad_img.data_ptr() if need_img else None, 0, B, C, H, W,
                                                      torch.cuda.current_stream().cuda_stream)
        sstem_native.check(rc, "sstem_warp_bilinear_backward_f32")
        return grad_img, grad_flow


class DifferentiableSpatialTransformation(SpatialTransformation):
    """``SpatialTransformation`` under autograd.  When neither input requires a gradient (or autograd is off) no node is recorded and
    the call is the base class's; otherwise only the gradients ``needs_input_grad`` asks for are computed, in one entry call: the flow
    gradient bit-reproducibly, the image gradient by fp32 atomics (its last bits can differ from run to run, include/sstem_warp.h)."""

    def forward(self, moving_image, deformation_matrix):
        if not (torch.is_grad_enabled() and (moving_image.requires_grad or deformation_matrix.requires_grad)):
            return super(DifferentiableSpatialTransformation, self).forward(moving_image, deformation_matrix)
        if not moving_image.is_cuda or not deformation_matrix.is_cuda:
            raise NotImplementedError("the warp kernel is GPU-only")
        B, C, H, W = moving_image.shape
        assert tuple(deformation_matrix.shape) == (B, H, W, 2)
        return _BackWarp.apply(moving_image.float().contiguous(), deformation_matrix.permute(0, 3, 1, 2).float().contiguous())
