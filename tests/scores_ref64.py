"""Float64 restatement, on torch, of the reference's validation scores -- compute_psnr / compute_ssim of utils/psnr_ssim.py:7-71 and EPE
of loss/multiscaleloss.py:5-16 -- and the recipes of the cases of tests/golden/scores.npz.  Used only by tests; CPU or GPU.

The SSIM window is the 2-D window exactly as the reference builds it (matlab_style_gauss2D with its eps cut, then the second
normalisation of compute_ssim), applied 'valid'; the branches are the reference's: both maxima <= 1 selects mean((a - b)^2) and the
quantisation (im * 255).astype(np.uint8), anything else mean((a / 255 - b / 255)^2) and the values as they are.  Where the reference
keeps float32 arrays in float32 (compute_psnr's square and mean, compute_ssim's three products in the `> 1` branch, EPE) this is
float64: the fixture records how far the reference is from it.  A negative value in the unit-range branch quantises to 0 (the
reference is undefined there).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

SENTINEL = 1000000000000         # compute_psnr's return where mse < 1e-10

# name -> (kind, H, W); "f32": a float32 pair in [0, 1]; "same": one image twice; "over1": a pair on the 1/4096 grid, one value 1.5;
# "u8": bytes of a float pair; "bits": bytes of 0 and 1
IMAGE_CASES = {
    "f11x11": ("f32", 11, 11),       # a one-element map
    "f11x43": ("f32", 11, 43),
    "f42x42": ("f32", 42, 42),       # a 32 x 32 map: whole tiles only
    "f43x44": ("f32", 43, 44),       # the first partial tiles
    "f75x53": ("f32", 75, 53),
    "same": ("same", 43, 44),
    "over1": ("over1", 43, 44),
    "u43x44": ("u8", 43, 44),
    "u75x53": ("u8", 75, 53),
    "bits": ("bits", 43, 44),
}
# name -> (shape, kind); "dense": no target pixel is (0, 0); "holes": about a third are; "empty": every one is
FLOW_CASES = {
    "small_dense": ((1, 2, 7, 9), "dense"),
    "small_holes": ((1, 2, 7, 9), "holes"),
    "small_empty": ((1, 2, 7, 9), "empty"),
    "wide_dense": ((3, 2, 33, 70), "dense"),
    "wide_holes": ((3, 2, 33, 70), "holes"),
}


def _seed(name):
    return 9100 + sum((i + 1) * ord(c) for i, c in enumerate(name))


def make_pair(H, W, seed):
    """Two float32 images in [0, 1]: one smooth image plus independent noise each, so that SSIM is neither near 0 nor near 1."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    smooth = 0.5 + 0.3 * np.sin(yy / 5.0 + rng.uniform(0, 6)) * np.cos(xx / 7.0 + rng.uniform(0, 6))
    a = np.clip(smooth + 0.05 * rng.standard_normal((H, W)), 0, 1).astype(np.float32)
    b = np.clip(smooth + 0.05 * rng.standard_normal((H, W)), 0, 1).astype(np.float32)
    return a, b


def make_image_case(name):
    kind, H, W = IMAGE_CASES[name]
    a, b = make_pair(H, W, _seed(name))
    if kind == "same":
        return a, a.copy()
    if kind == "over1":
        # values k / 4096: every product of two of them has at most 24 significant bits, so the float32 products the reference forms in
        # this branch are exact and its SSIM is a float64 computation like ref64's
        a, b = (np.round(a * 4096) / 4096).astype(np.float32), (np.round(b * 4096) / 4096).astype(np.float32)
        a[3, 5] = 1.5
        return a, b
    if kind == "u8":
        return (a * 255).astype(np.uint8), (b * 255).astype(np.uint8)
    if kind == "bits":
        rng = np.random.default_rng(_seed(name) + 1)
        bits = (a > 0.5).astype(np.uint8)
        flip = (rng.random((H, W)) < 0.1).astype(np.uint8)
        return bits, bits ^ flip
    return a, b


def make_flow_case(name):
    shape, kind = FLOW_CASES[name]
    rng = np.random.default_rng(_seed(name))
    flow = (2.0 * rng.standard_normal(shape)).astype(np.float32)
    target = (flow + 0.5 * rng.standard_normal(shape)).astype(np.float32)
    if kind == "holes":
        hole = rng.random((shape[0], 1, shape[2], shape[3])) < 0.33
        target = np.where(hole, np.float32(0), target).astype(np.float32)
    elif kind == "empty":
        target = np.zeros(shape, dtype=np.float32)
    return flow, target


def window2d(device="cpu"):
    """matlab_style_gauss2D((11, 11), 1.5) and compute_ssim's second normalisation, in float64."""
    r = torch.arange(-5, 6, dtype=torch.float64, device=device)
    h = torch.exp(-(r[None, :] * r[None, :] + r[:, None] * r[:, None]) / (2.0 * 1.5 * 1.5))
    h = torch.where(h < torch.finfo(torch.float64).eps * h.max(), torch.zeros_like(h), h)
    h = h / h.sum()
    return h / h.sum()


def unit_range(a, b):
    """np.max(img1) <= 1.0 and np.max(img2) <= 1.0 (a NaN maximum is not <= 1)."""
    return bool(a.max() <= 1) and bool(b.max() <= 1)


def _quantise(x):
    if x.dtype == torch.uint8:
        return x * 255                       # numpy keeps uint8 here; reached by images of 0 and 1 only
    return (x.clamp_min(0) * 255.0).to(torch.uint8)          # float32 multiply, truncation


def psnr64(a, b):
    """-> (mse, psnr) as Python floats; psnr is 1e12 where the reference returns its bare sentinel."""
    x, y = a.double(), b.double()
    mse = float(((x - y) ** 2).mean()) if unit_range(a, b) else float(((x / 255.0 - y / 255.0) ** 2).mean())
    if mse < 1.0e-10:
        return mse, 1.0e12
    return mse, 20 * math.log10(1 / math.sqrt(mse))


def ssim64(a, b):
    if unit_range(a, b):
        a, b = _quantise(a), _quantise(b)
    x, y = a.double()[None, None], b.double()[None, None]
    w = window2d(x.device)[None, None]
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    mu1, mu2 = F.conv2d(x, w), F.conv2d(y, w)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1 = F.conv2d(x * x, w) - mu1_sq
    s2 = F.conv2d(y * y, w) - mu2_sq
    s12 = F.conv2d(x * y, w) - mu1_mu2
    m = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return float(m.mean())


def score64(a, b, clamp01=False):
    """[B,3] float64 (mse, psnr, ssim) of a batch [B,H,W], image by image; clamp01 clamps a to [0, 1] first."""
    rows = []
    for i in range(a.shape[0]):
        x = a[i].clamp(0, 1) if clamp01 else a[i]
        rows.append(list(psnr64(x, b[i])) + [ssim64(x, b[i])])
    return torch.tensor(rows, dtype=torch.float64)


def epe64(flow, target, sparse=False, mean=True):
    d = (target.double() - flow.double())
    m = torch.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    if sparse:
        m = m[~((target[:, 0] == 0) & (target[:, 1] == 0))]
    return float(m.mean()) if mean else float(m.sum()) / flow.shape[0]
