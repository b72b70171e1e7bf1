"""Generates tests/golden/jitter.npz from PIL (recorded with Pillow 12.2.0; ``pil_version`` in the file says which) and from the REFERENCE's
fusion provider (sff_scripts_fusion/data/data_provider.py), imported in place from the reference tree (nothing is copied), on the CPU.

The file holds, with the cases and the seeded images of tests/jitter_ref.py (the images are not stored):
  (a) ``blend`` uint8 [factor, d, 256]: np.asarray(Image.blend(Image.new("L", (256, 1), d), ramp, f)) for every d in 0..255 and every f of
      jitter_ref.BLEND_FACTORS, ramp the bytes 0..255;
  (b) ``c<chain>_<image>`` uint8: the image after the ImageEnhance chain jitter_ref.CHAINS[chain] (Brightness, Contrast, Color);
  (c) per seed of jitter_ref.PROVIDER_SEEDS: ``p<seed>_im`` [6,d,d], ``_lb`` [1,d,d] float32 as the fusion provider's ``__getitem__``
      returned them after random.seed(seed) with color_jitter on (gt_line on for odd seeds), ``_steps`` [k,2] float64 (op code, factor)
      as drawn, ``_drawn`` the number of candidate folds, and ``_next``, what random.random() gave right after.

Interventions in (c), on top of make_crop_batch_golden.py's stand-in object: torchvision is not installed here, so the provider's ``cj``
is bound to ``_ColorJitterStandIn`` below -- a STAND-IN for torchvision.transforms.ColorJitter(b, c, s, hue=0), not torchvision: it draws
from the provider's ``random`` module as tests/jitter_ref.draw_jitter states (torchvision 0.2's get_params, restated from memory of its
source: this order is unpinned) and applies PIL's own ImageEnhance classes, which is what torchvision's adjust_brightness /
adjust_contrast / adjust_saturation call.  The provider's own ``_color_jitter`` (Image.fromarray, np.asarray) runs unchanged.

    python tests/golden/make_jitter_golden.py [out.npz]
"""
import os
import sys
import types

import numpy as np
import PIL
from PIL import Image, ImageEnhance

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import crop_ref as C  # noqa: E402
import jitter_ref as J  # noqa: E402
import make_crop_batch_golden as M  # noqa: E402
import make_fold_golden as F  # noqa: E402

ENHANCERS = {J.BRIGHTNESS: ImageEnhance.Brightness, J.CONTRAST: ImageEnhance.Contrast, J.SATURATION: ImageEnhance.Color}


def reference_available():
    return M.reference_available()


def enhance_chain(img, steps):
    """PIL's own chain on the uint8 array `img`."""
    pil = Image.fromarray(img)
    assert pil.mode == "L"
    for code, factor in steps:
        pil = ENHANCERS[code](pil).enhance(factor)
    return np.asarray(pil).copy()


class _ColorJitterStandIn(object):
    """Stand-in for the absent torchvision.transforms.ColorJitter(brightness, contrast, saturation, hue=0); see the module's docstring."""

    def __init__(self, rng, brightness, contrast, saturation):
        self.rng, self.strengths, self.drawn = rng, (brightness, contrast, saturation), []

    def __call__(self, pil):
        steps = []
        for code, x in zip((J.BRIGHTNESS, J.CONTRAST, J.SATURATION), self.strengths):
            if x > 0:
                steps.append((code, self.rng.uniform(max(0, 1 - x), 1 + x)))
        self.rng.shuffle(steps)
        self.drawn.append(steps)
        for code, factor in steps:
            pil = ENHANCERS[code](pil).enhance(factor)
        return pil


def generate():
    out = {"pil_version": np.array(PIL.__version__)}
    # (a) exhaustive blends
    ramp = Image.fromarray(np.arange(256, dtype=np.uint8)[None, :])
    blend = np.empty((len(J.BLEND_FACTORS), 256, 256), dtype=np.uint8)
    for fi, f in enumerate(J.BLEND_FACTORS):
        for d in range(256):
            blend[fi, d] = np.asarray(Image.blend(Image.new("L", (256, 1), d), ramp, f))[0]
    out["blend"] = blend
    # (b) chains
    for ci, steps in enumerate(J.CHAINS):
        for name, img in J.images().items():
            out["c%d_%s" % (ci, name)] = enhance_chain(img, steps)
    # (c) the fusion provider, degradation and _color_jitter bound, gen_flow counted
    _, _, fusion = F._reference_modules()
    calls = [0]
    gen_flow = fusion.gen_flow

    def counted(*a, **kw):
        calls[0] += 1
        return gen_flow(*a, **kw)

    fusion.gen_flow = counted
    images = C.images_of(C.FUSION_IMAGES)
    offset = (C.FUSION_CROP[0] - C.FUSION_DET) // 2
    drawn = []
    for seed in J.PROVIDER_SEEDS:
        obj = M._stand_in(C.FUSION_FLAGS, C.FUSION_CROP, len(C.FUSION_PAIRS), None, interp_train_list=list(range(len(C.FUSION_PAIRS))),
                          det_size=C.FUSION_DET, offset=offset, gt_line=bool(seed & 1))
        obj.color_jitter = True
        obj.cj = _ColorJitterStandIn(fusion.random, *J.PROVIDER_JITTER)
        obj.read_img = lambda a, b: (images[C.FUSION_PAIRS[a][0]], images[C.FUSION_PAIRS[b][1]])
        obj.degradation = types.MethodType(fusion.Train.degradation, obj)
        obj._color_jitter = types.MethodType(fusion.Train._color_jitter, obj)
        calls[0] = 0
        fusion.random.seed(seed)
        im, lb = fusion.Train.__getitem__(obj, 0)
        key = "p%d_" % seed
        out[key + "im"], out[key + "lb"], out[key + "next"] = im, lb, np.float64(fusion.random.random())
        assert len(obj.cj.drawn) == 1 and len(obj.cj.drawn[0]) == 3
        out[key + "steps"] = np.array(obj.cj.drawn[0], dtype=np.float64)
        out[key + "drawn"] = np.int64(calls[0])
        drawn.append(calls[0])
        assert im.dtype == np.float32 and lb.dtype == np.float32 and im.shape == (6, C.FUSION_DET, C.FUSION_DET) and lb.shape == (1, C.FUSION_DET, C.FUSION_DET)
    assert max(drawn) > 1, "one seed must reject its first fold: %s" % drawn
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "jitter.npz")
    data = generate()
    np.savez_compressed(path, **data)
    print("arrays:", len(data), "PIL", PIL.__version__)
    print("candidate folds per provider seed:", [int(data["p%d_drawn" % s]) for s in J.PROVIDER_SEEDS])
    print("wrote", path, os.path.getsize(path), "bytes; crop_batch.npz is", os.path.getsize(os.path.join(HERE, "crop_batch.npz")))
