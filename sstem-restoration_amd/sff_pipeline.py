"""SFF restoration forward (interpolation + unfolding flow + fusion) for a batch of tiles, and its tile-sharded driver --
the literal wording of the headline metric, "interp + fusion fwd".

Dataflow of the reference's SFF inference scripts:

    interp  = IFNet(cat(prev x3, next x3))                      sff_scripts_interp/inference_singleImage.py:55-71
    inputs  = cat(sff x3, interp x3)                            sff_scripts_fusion/inference.py:126-136
    flow    = FusionNet(6, 2, 32)(inputs)                       :142  (the unfolding flow predictor, eval)
    warped  = SpatialTransformation(inputs[:, :3], flow.permute(0, 2, 3, 1))    :145-150
    inputs[:, :3] = warped ;  pred = UNet(6, 1)(inputs)         :152-153  (the fusion net, eval)

The reference writes the interpolated frame to a PNG between the two scripts (uint8 truncation, utils of f3); here the chain
stays on the GPU in fp32 -- ``quantise_interp=True`` reproduces the PNG round trip (``(x*255).astype(uint8) / 255``) for callers
that want the files' arithmetic.  Tiles are independent: ranks own tiles round-robin, weights are broadcast once.
"""
import torch

import dataparallel as dp
import sstem_native
from model.model_fusionnet import FusionNet
from model.model_interp import IFNet
from model.model_unet import UNet
from utils.flow_display import flow_color_batch
from utils.image_warp_torch import SpatialTransformation

_warp = SpatialTransformation(use_gpu=True)


def _png_round_trip(t):
    """(t*255).astype(uint8) / 255 with the native edge kernels (include/sstem_io.h: numpy's truncation, no clamp)."""
    t = t.contiguous()
    u8 = torch.empty(t.shape, dtype=torch.uint8, device=t.device)
    out = torch.empty_like(t)
    lib = sstem_native.load_library()
    with torch.cuda.device(t.device):
        s = torch.cuda.current_stream().cuda_stream
        sstem_native.check(lib.sstem_f32_to_gray_u8(t.data_ptr(), u8.data_ptr(), t.numel(), 0, s), "sstem_f32_to_gray_u8")
        sstem_native.check(lib.sstem_gray_u8_to_f32(u8.data_ptr(), out.data_ptr(), t.numel(), 1, s), "sstem_gray_u8_to_f32")
    return out


def build_models(device):
    return {"interp": IFNet(51).eval().to(device), "flow": FusionNet(6, 2, 32).eval().to(device),
            "fusion": UNet(6, 1).eval().to(device)}


@torch.no_grad()
def interpolate(models, prev, nxt, quantise_interp=False):
    """Stage 1 (inference_singleImage.py:55-76): the interpolated section [B,1,H,W]; ``quantise_interp`` = the PNG the reference
    writes between its two scripts (*255, uint8 truncation without clamp, /255 on reading)."""
    interp = models["interp"].interpolate_gray(prev, nxt)
    return _png_round_trip(interp) if quantise_interp else interp


@torch.no_grad()
def fuse(models, sff, interp):
    """Stage 2 (sff_scripts_fusion/inference.py:126-153): flow on cat(sff x3, interp x3), back-warp of the SFF channels, fusion UNet.
    Returns (pred [B,1,H,W], flow [B,2,H,W], warped_sff [B,3,H,W])."""
    B, _, H, W = sff.shape
    inputs = torch.cat((sff.expand(B, 3, H, W), interp.expand(B, 3, H, W)), 1)
    flow = models["flow"](inputs)
    warped = _warp(inputs[:, :3], flow.permute(0, 2, 3, 1))
    inputs[:, :3] = warped
    pred = models["fusion"](inputs)
    return pred, flow, warped


@torch.no_grad()
def restore_sff(models, prev, nxt, sff, quantise_interp=False):
    """prev, nxt: the neighbouring sections; sff: the folded section; float32 [B,1,H,W] in [0,1] on the GPU, H and W
    multiples of 32.  Returns (pred [B,1,H,W], interp [B,1,H,W], flow [B,2,H,W], warped_sff [B,3,H,W])."""
    interp = interpolate(models, prev, nxt, quantise_interp)
    pred, flow, warped = fuse(models, sff, interp)
    return pred, interp, flow, warped


def _planes(t, name, channels, dtype):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise NotImplementedError("sff_pipeline.outputs is GPU-only: %s must be a GPU tensor" % name)
    if t.dtype != dtype:
        raise TypeError("sff_pipeline.outputs: %s must be %s (got %s)" % (name, dtype, t.dtype))
    if channels == 1 and t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != (3 if channels == 1 else 4) or (channels != 1 and t.shape[1] != channels):
        raise ValueError("sff_pipeline.outputs: %s has shape %r" % (name, tuple(t.shape)))
    return t.contiguous()


@torch.no_grad()
def outputs(pred, warped, interp_u8, flow=None):
    """The images the two inference scripts save (sff_scripts_fusion/inference.py:161-172, sff_scripts_unfolding/inference.py:146-153),
    made on the device (``include/sstem_display.h``): one launch for the images, two for the flow.
    pred [B,1,H,W] or [B,H,W] and warped [B,3,H,W] float32 as ``fuse`` returns them, interp_u8 [B,H,W] or [B,1,H,W] uint8 -- the
    interpolated section as the script read it from its file.  Returns
    (pred_u8 [B,H,W], warped_rgb [B,H,W,3], stitch [B,H,W]) uint8, and as a fourth the colour image [B,H,W,3] of flow [B,2,H,W] when
    it is given.  pad: 0, as in every shipped configuration.  Nothing synchronises."""
    pred, warped, interp_u8 = _planes(pred, "pred", 1, torch.float32), _planes(warped, "warped", 3, torch.float32), _planes(interp_u8, "interp_u8", 1, torch.uint8)
    B, H, W = pred.shape
    if warped.shape != (B, 3, H, W) or interp_u8.shape != (B, H, W) or warped.device != pred.device or interp_u8.device != pred.device:
        raise ValueError("sff_pipeline.outputs: pred %r, warped %r and interp_u8 %r do not belong together"
                         % (tuple(pred.shape), tuple(warped.shape), tuple(interp_u8.shape)))
    pred_u8 = torch.empty((B, H, W), dtype=torch.uint8, device=pred.device)
    warped_rgb = torch.empty((B, H, W, 3), dtype=torch.uint8, device=pred.device)
    stitch = torch.empty((B, H, W), dtype=torch.uint8, device=pred.device)
    lib = sstem_native.load_library()
    with torch.cuda.device(pred.device):
        rc = lib.sstem_sff_outputs_u8(pred.data_ptr(), warped.data_ptr(), interp_u8.data_ptr(), B, H, W, pred_u8.data_ptr(),
                                      warped_rgb.data_ptr(), stitch.data_ptr(), torch.cuda.current_stream().cuda_stream)
    sstem_native.check(rc, "sstem_sff_outputs_u8")
    if flow is None:
        return pred_u8, warped_rgb, stitch
    return pred_u8, warped_rgb, stitch, flow_color_batch(flow)


def restore_sharded(models, tiles, rank, world):
    """tiles: list of (prev, next, sff) GPU tensors (or callables producing them).  Weights must already be identical on every
    rank (``dataparallel.broadcast_module``).  Returns {index: pred} for the tiles this rank owns."""
    out = {}
    for idx in dp.shard_indices(len(tiles), rank, world):
        t = tiles[idx]
        if callable(t):
            t = t()
        out[idx] = restore_sff(models, *t)[0]
    return out
