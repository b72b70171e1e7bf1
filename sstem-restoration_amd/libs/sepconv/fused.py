"""``interp_apply`` -- the IFNet epilogue as one native launch (include/sstem_sepconv.h).

    out = mean_c( sepconv(ReplicationPad2d(25)(i2), k2v, k2h) + sepconv(ReplicationPad2d(25)(i1), k1v, k1h) )

i.e. ``sff_scripts_interp/model/model_interp.py:90-97`` (and each output channel of
``sp_scripts_train/networks.py:116-124``).  Forward only: the models use it when autograd is off and keep
the separate ``SeparableConvolution`` op (which has a backward) for training.  GPU tensors only.
"""
import torch

import sstem_native


def _apply(name, entry, ts, planes, coef_dtype=torch.float32, layout="nchw", copy=True, u8=False):
    """The five wrappers below.  ts: two frames of `planes` channels and four coefficient tensors of `coef_dtype`, [B,51,H,W]
    ("nchw"), ``coef_blocked_shape`` ("blocked") or whichever of the two they have ("either").  copy: non-contiguous tensors are
    copied, else refused.  u8: the entry also stores the uint8 image and takes the layout as a flag."""
    if coef_dtype is torch.bfloat16:
        needs = "float32 planes and bfloat16 coefficient tensors"
    else:
        needs = "float32 tensors" if copy else "contiguous float32 tensors"
    for t, dtype in zip(ts, [torch.float32] * 2 + [coef_dtype] * 4):
        if not t.is_cuda:
            raise NotImplementedError("%s is GPU-only" % name)
        if t.dtype != dtype or not (copy or t.is_contiguous()):
            raise TypeError("%s needs %s" % (name, needs))
    B, C, H, W = ts[0].shape
    blocked = layout == "blocked" or (layout == "either" and ts[2].dim() == 5)
    want = coef_blocked_shape(B, H, W) if blocked else (B, 51, H, W)
    if C != planes or tuple(ts[1].shape) != (B, planes, H, W) or any(tuple(k.shape) != want for k in ts[2:]):
        raise RuntimeError("%s: inconsistent shapes" % name)
    if copy:
        ts = [t.contiguous() for t in ts]
    outs = [ts[0].new_empty((B, 1, H, W))]
    if u8:
        outs.append(torch.empty((B, H, W), dtype=torch.uint8, device=ts[0].device))
    args = [t.data_ptr() for t in ts + outs] + [B, H, W] + ([1 if blocked else 0] if u8 else [])
    with torch.cuda.device(ts[0].device):
        rc = getattr(sstem_native.load_library(), entry)(*args, torch.cuda.current_stream().cuda_stream)
    sstem_native.check(rc, entry)
    return tuple(outs) if u8 else outs[0]


def interp_apply(i1, i2, k1v, k1h, k2v, k2h):
    return _apply("interp_apply", "sstem_sepconv_interp_apply_f32", [i1, i2, k1v, k1h, k2v, k2h], planes=3)


def interp_apply_gray_supported(B, H, W):
    return bool(sstem_native.load_library().sstem_sepconv_interp_apply_gray_supported(B, H, W))


def interp_apply_gray(g1, g2, k1v, k1h, k2v, k2h):
    """The same apply for callers that built the x3 channel replication themselves (every caller of the reference does:
    inference_singleImage.py:55-61, test_fusion.py:105-106): g1, g2 are the single planes [B,1,H,W].  Bit-identical to
    ``interp_apply`` on the replicated frames; one launch, no channel comparison (include/sstem_sepconv.h)."""
    return _apply("interp_apply_gray", "sstem_sepconv_interp_apply_gray_f32", [g1, g2, k1v, k1h, k2v, k2h], planes=1)


# ---- blocked coefficients (include/sstem_sepconv.h): [B, H, ceil(W/64), 51, 64] -----------------------------------------------

def coef_blocked_shape(B, H, W):
    return (B, H, (W + 63) // 64, 51, 64)


def interp_apply_gray_blocked_supported(B, H, W):
    return bool(sstem_native.load_library().sstem_sepconv_interp_apply_gray_blocked_supported(B, H, W))


def coef_to_blocked(coef):
    """NCHW coefficients [B,51,H,W] -> the row-segment layout the blocked apply reads (tests, foreign producers; the IFNet's
    kernel heads store that layout themselves)."""
    if not coef.is_cuda:
        raise NotImplementedError("coef_to_blocked is GPU-only")
    if coef.dtype != torch.float32 or coef.dim() != 4 or coef.shape[1] != 51:
        raise RuntimeError("coef_to_blocked needs a float32 [B,51,H,W] tensor")
    coef = coef.contiguous()
    B, _, H, W = coef.shape
    out = coef.new_empty(coef_blocked_shape(B, H, W))
    with torch.cuda.device(coef.device):
        rc = sstem_native.load_library().sstem_sepconv_coef_to_blocked_f32(coef.data_ptr(), out.data_ptr(), B, H, W,
                                                                           torch.cuda.current_stream().cuda_stream)
    sstem_native.check(rc, "sstem_sepconv_coef_to_blocked_f32")
    return out


def interp_apply_gray_blocked(g1, g2, k1v, k1h, k2v, k2h):
    """``interp_apply_gray`` on coefficient tensors in the blocked layout: bit-identical output, the coefficient streams walk
    consecutive addresses."""
    return _apply("interp_apply_gray_blocked", "sstem_sepconv_interp_apply_gray_blocked_f32", [g1, g2, k1v, k1h, k2v, k2h], planes=1,
                  layout="blocked", copy=False)


# ---- bfloat16 coefficient tensors (include/sstem_sepconv.h, ..._bf16coef) ------------------------------------------------------

def interp_apply_gray_bf16coef_supported(B, H, W):
    return bool(sstem_native.load_library().sstem_sepconv_interp_apply_gray_bf16coef_supported(B, H, W))


def interp_apply_gray_bf16coef(g1, g2, k1v, k1h, k2v, k2h):
    """``interp_apply_gray`` on bfloat16 coefficient tensors [B,51,H,W] (the kernel heads' outputs handed over in bf16: half the
    coefficient bytes); planes, sums and the result float32 -- bit for bit what ``interp_apply_gray`` returns on ``k.float()``."""
    return _apply("interp_apply_gray_bf16coef", "sstem_sepconv_interp_apply_gray_bf16coef", [g1, g2, k1v, k1h, k2v, k2h], planes=1,
                  coef_dtype=torch.bfloat16)


# ---- the uint8 image stored by the apply itself (include/sstem_sepconv.h, sstem_sepconv_interp_apply_gray_u8_f32) --------------

def interp_apply_gray_u8(g1, g2, k1v, k1h, k2v, k2h):
    """``interp_apply_gray`` / ``interp_apply_gray_blocked`` (by the coefficient tensors' shape) that ALSO returns
    ``(out * 255).astype(uint8)`` -- numpy's truncation, no clamp (inference_singleImage.py:76) -- stored by the same launch:
    (out float32 [B,1,H,W], image uint8 [B,H,W])."""
    return _apply("interp_apply_gray_u8", "sstem_sepconv_interp_apply_gray_u8_f32", [g1, g2, k1v, k1h, k2v, k2h], planes=1,
                  layout="either", copy=False, u8=True)
