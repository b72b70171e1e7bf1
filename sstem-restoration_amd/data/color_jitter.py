"""The colour jitter of the SFF fusion and unfolding providers (``sff_scripts_fusion/data/data_provider.py:146-148,309-313``) on the
device: ``torchvision.transforms.ColorJitter(brightness, contrast, saturation, hue=0)`` on a 2-D uint8 crop is a chain of PIL
``ImageEnhance`` blends, each a map from byte to byte, so a sample's whole jitter is one 256-entry table
(``include/sstem_jitter.h``).  The host draws the factors and their order (``draw_jitter``); ``jitter_luts`` makes every sample's table in
one entry call, and ``data.fold_degradation.degrade(..., lut=)`` reads the section through it -- bit for bit PIL's bytes.

    steps = [draw_jitter(random, 0.5, 0.5, 0.5) for _ in range(B)]
    lut = jitter_luts(clean_u8, steps)                        # [B, 256] uint8 on the GPU
    jittered = torch.gather(lut, 1, clean_u8.reshape(B, -1).long()).reshape(clean_u8.shape)      # what the table means

GPU tensors only -- there is no CPU fallback.
"""
import numpy as np
import torch

import sstem_native

JITTER_OPS = 4            # SSTEM_JITTER_OPS of include/sstem_jitter.h
NONE, BRIGHTNESS, CONTRAST, SATURATION = 0, 1, 2, 3


def draw_jitter(rng, brightness, contrast, saturation):
    """One sample's steps ``[(code, factor), ...]`` in the order they are applied, from ``rng`` (a ``random.Random`` or the ``random``
    module), consuming it as ``ColorJitter.get_params`` of torchvision 0.2 does (the version the reference's docker pins beside torch
    0.4): per nonzero strength x, in the order brightness, contrast, saturation, one ``rng.uniform(max(0, 1 - x), 1 + x)``; then one
    ``rng.shuffle`` of the list.  Hue 0 draws nothing.

    UNPINNED: torchvision is not installed where this was written, so the draw order is restated from memory of its source and no
    fixture holds torchvision's own draws.  The arithmetic of the steps is pinned against PIL (``tests/golden/jitter.npz``)."""
    steps = []
    for code, x in ((BRIGHTNESS, brightness), (CONTRAST, contrast), (SATURATION, saturation)):
        if x > 0:
            steps.append((code, rng.uniform(max(0, 1 - x), 1 + x)))
    rng.shuffle(steps)
    return steps


def step_tables(steps):
    """Per-sample step lists -> (codes ``[n, JITTER_OPS]`` int32, factors ``[n, JITTER_OPS]`` float32) host arrays, validated: at most
    JITTER_OPS steps per sample, codes in [0, 3]; short lists are padded with (NONE, 0)."""
    n = len(steps)
    codes = np.zeros((n, JITTER_OPS), dtype=np.int32)
    factors = np.zeros((n, JITTER_OPS), dtype=np.float32)
    for i, sample in enumerate(steps):
        if len(sample) > JITTER_OPS:
            raise ValueError("sample %d has %d jitter steps, at most %d fit" % (i, len(sample), JITTER_OPS))
        for q, (code, factor) in enumerate(sample):
            if code not in (NONE, BRIGHTNESS, CONTRAST, SATURATION):
                raise ValueError("sample %d step %d: unknown jitter op %r" % (i, q, code))
            codes[i, q], factors[i, q] = code, factor
    return codes, factors


def jitter_luts(planes_u8, steps):
    """``[n, 256]`` uint8 GPU tensor: row i is sample i's table for ``planes_u8[i]`` (``[n, S_h, S_w]`` uint8 GPU tensor) under
    ``steps[i]``.  One upload of the two small tables, one entry call (three launches), no synchronisation."""
    if not isinstance(planes_u8, torch.Tensor) or not planes_u8.is_cuda:
        raise NotImplementedError("the jitter kernels are GPU-only")
    assert planes_u8.dtype == torch.uint8 and planes_u8.dim() == 3 and planes_u8.is_contiguous()
    n, S_h, S_w = planes_u8.shape
    if len(steps) != n:
        raise ValueError("%d step lists for %d planes" % (len(steps), n))
    codes, factors = step_tables(steps)
    dev = planes_u8.device
    # both tables travel in one int32 tensor: the codes, then the factors' bits
    flat = torch.from_numpy(np.concatenate([codes.reshape(-1), factors.reshape(-1).view(np.int32)])).to(dev)
    op_code, op_factor = flat[:n * JITTER_OPS], flat[n * JITTER_OPS:].view(torch.float32)
    lut = torch.empty((n, 256), dtype=torch.uint8, device=dev)
    hist = torch.empty((n, 256), dtype=torch.int32, device=dev)              # workspace: the entry clears it
    lib = sstem_native.load_library()
    with torch.cuda.device(dev):
        rc = lib.sstem_jitter_lut_u8(planes_u8.data_ptr(), n, S_h, S_w, op_code.data_ptr(), op_factor.data_ptr(), lut.data_ptr(),
                                     hist.data_ptr(), torch.cuda.current_stream().cuda_stream)
    sstem_native.check(rc, "sstem_jitter_lut_u8")
    return lut
