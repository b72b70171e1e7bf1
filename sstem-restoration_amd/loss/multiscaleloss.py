"""``EPE`` / ``realEPE`` -- the reference's flow end-point error on MI355X.

Mirrors ``loss/multiscaleloss.py:5-16,57-60`` of the reference (``from loss.multiscaleloss import EPE, realEPE``): the validation
number of the flow network (sff_scripts_unfolding/main_flowfusionnet.py:279) and of the correction stage's inference
(sff_scripts_unfolding/inference.py:135).  One native launch (``include/sstem_score.h``, ``csrc/score_kernels.hip``): per-pixel
``sqrt(dx^2 + dy^2)`` and its sum in float64, in a fixed order; the result is a float32 0-d GPU tensor, the reference's dtype, and
nothing synchronises.

* ``[B,2,H,W]`` float32 GPU tensors; a CPU tensor raises ``NotImplementedError``, other channel counts ``ValueError``.
* ``realEPE`` handles the same-size case -- what the FusionNet flow predictor produces, where the reference's bilinear
  ``align_corners=False`` resize to the same size is the identity.  Another size raises ``NotImplementedError``: the up-sampling
  belongs to flownet-style models that the reference tree does not contain either.
* ``multiscaleEPE`` and ``sparse_max_pool`` are not here: no loop of the reference calls them.
"""
import torch

import sstem_native
from utils import psnr_ssim


def _check_flows(input_flow, target_flow):
    for t in (input_flow, target_flow):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise NotImplementedError("EPE is GPU-only")
    if input_flow.dtype != torch.float32 or target_flow.dtype != torch.float32:
        raise TypeError("EPE: float32 flows")
    if input_flow.dim() != 4 or input_flow.shape[1] != 2 or input_flow.shape != target_flow.shape:
        raise ValueError("EPE: two [B,2,H,W] flows of one shape, got %r and %r" % (tuple(input_flow.shape), tuple(target_flow.shape)))


def _epe_float64(input_flow, target_flow, sparse, mean):
    """The launch's own result: a float64 0-d GPU tensor."""
    _check_flows(input_flow, target_flow)
    lib = sstem_native.load_library()
    f, t = input_flow.detach().contiguous(), target_flow.detach().contiguous()
    B, _, H, W = f.shape
    value = torch.empty((), dtype=torch.float64, device=f.device)
    with torch.cuda.device(f.device):
        ws = psnr_ssim._workspace(lib, B, H, W, f.device)
        rc = lib.sstem_flow_epe_f32(f.data_ptr(), t.data_ptr(), B, H, W, 1 if sparse else 0, 1 if mean else 0, value.data_ptr(),
                                    ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    sstem_native.check(rc, "sstem_flow_epe_f32")
    return value


def EPE(input_flow, target_flow, sparse=False, mean=True):
    return _epe_float64(input_flow, target_flow, sparse, mean).to(torch.float32)


def realEPE(output, target, sparse=False):
    if isinstance(output, torch.Tensor) and isinstance(target, torch.Tensor) and output.dim() == 4 and target.dim() == 4 \
            and output.shape[2:] != target.shape[2:]:
        raise NotImplementedError("realEPE: the bilinear up-sampling of the output to the target's size %r is not implemented (got %r)"
                                  % (tuple(target.shape[2:]), tuple(output.shape[2:])))
    return EPE(output, target, sparse, mean=True)
