"""``gen_line`` / ``gen_flow`` -- the reference's synthetic fold flow (``sff_scripts_fusion/utils/flow_synthesis.py:8-87``) on MI355X.

Same names and arguments; ``gen_flow`` returns GPU tensors instead of numpy arrays: ``flow`` and ``flow2`` ``[H,W,2]`` float32 and
``mask`` ``[H,W]`` float64, bit for bit what the reference computes in ~30 float64 numpy passes, from one native launch
(``include/sstem_fold.h``).  The fold's scalars are derived here, on the host, with the reference's own Python expressions
(``fold_scalars``); the kernel does the per-pixel part.  GPU only -- there is no CPU fallback.
"""
import math

import torch

import sstem_native

mina = 0.000000001

FOLD_PARAMS = 10          # SSTEM_FOLD_PARAMS of include/sstem_fold.h


def gen_line(p1, p2):
    denominator = p2[1] - p1[1]
    if denominator == 0:
        denominator = mina
    k = (p2[0] - p1[0]) / denominator
    b = p1[0] - (k * p1[1])
    return k, b


def fold_scalars(k, b, line_width=5, fold_width=10, dis_k=0.1):
    """The fold as the row of doubles the kernels take (layout: include/sstem_fold.h)."""
    norm = math.sqrt(k ** 2 + 1)
    ndk = -dis_k
    dis_b = (fold_width - line_width) - ndk * line_width
    if k == 0:
        k_T = 1 / mina
    else:
        k_T = 1 / k
    angle = math.atan(k_T)
    sin_p = math.sin(angle)
    cos_p = math.cos(angle)
    return [float(k), float(b), norm, float(line_width), float(fold_width), ndk, float(dis_b), cos_p, sin_p, 1.0 if k > 0 else 0.0]


def _device(device):
    if not torch.cuda.is_available():
        raise NotImplementedError("the fold kernels are GPU-only")
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise NotImplementedError("the fold kernels are GPU-only")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def gen_flow(height, width, k, b, line_width=5, fold_width=10, dis_k=0.1, device=None):
    dev = _device(device)
    folds = torch.tensor([fold_scalars(k, b, line_width, fold_width, dis_k)], dtype=torch.float64).to(dev)
    flow = torch.empty((height, width, 2), dtype=torch.float32, device=dev)
    flow2 = torch.empty_like(flow)
    mask = torch.empty((height, width), dtype=torch.uint8, device=dev)
    lib = sstem_native.load_library()
    with torch.cuda.device(dev):
        rc = lib.sstem_fold_flow(folds.data_ptr(), 1, height, width, flow.data_ptr(), flow2.data_ptr(), mask.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
    sstem_native.check(rc, "sstem_fold_flow")
    return flow, flow2, mask.to(torch.float64)
