"""Generates tests/golden/crop_batch.npz from the REFERENCE's data providers, imported in place from the reference tree (nothing is
copied), on the CPU:
  sff_scripts_interp/data/data_provider.py   Train.__getitem__   (the IFNet sample)
  sff_scripts_fusion/data/data_provider.py   Train.__getitem__ with Train.degradation bound   (the fusion sample)
  sp_scripts_train/dataset.py                ImageDataset.RotationFlip   (the eight cases)

Interventions, the pattern of make_fold_golden.py: whichever of the providers' top-level imports is not installed here (cv2, h5py,
torchvision, tifffile, ...) is registered as an empty stand-in module while the file is imported -- the code run below touches none of
them.  ``__getitem__`` runs unbound on a stand-in object that carries only what it reads: the crop size, the augmentation flags, the
list length and a ``read_img`` that returns the seeded images of tests/crop_ref.py (the images are not stored).

The file holds:
  (a) per flag set ``<f>`` and seed ``<s>`` of crop_ref.INTERP_FLAG_SETS / INTERP_SEEDS: ``i_<f>_<s>_im`` [6,S,S], ``_lb`` [1,S,S] float32 as
      ``__getitem__`` returned them after random.seed(s), and ``_next``, the value random.random() gave right after (the stream's position);
  (b) per seed of crop_ref.FUSION_SEEDS: ``f_<s>_im`` [6,d,d], ``_lb`` [1,d,d] and ``_next`` of the fusion provider, gt_line on for odd seeds;
  (c) ``sp_case`` [8,n,n] uint8: RotationFlip(square, case) of crop_ref.SP_SQUARE.

    python tests/golden/make_crop_batch_golden.py [out.npz]
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import crop_ref as C  # noqa: E402
import make_fold_golden as F  # noqa: E402

REF_INTERP = os.path.join(F.REF, "sff_scripts_interp", "data", "data_provider.py")
REF_SP = os.path.join(F.REF, "sp_scripts_train", "dataset.py")

STAND_INS = ("cv2", "h5py", "torchvision", "torchvision.transforms", "tifffile", "joblib", "scipy.ndimage.interpolation",
             "scipy.ndimage.filters", "utils", "utils.util")


def reference_available():
    return F.reference_available() and os.path.exists(REF_INTERP) and os.path.exists(REF_SP)


def _load_with_stand_ins(name, path, always=()):
    """Imports `path` with every module of STAND_INS that does not import here (and every one of `always`) replaced by a stand-in."""
    saved, added = {}, []
    for mod in STAND_INS:
        if mod not in always:
            try:
                importlib.import_module(mod)
                continue
            except Exception:
                pass
        saved[mod] = sys.modules.get(mod)
        sys.modules[mod] = F._Stub(mod)
        added.append(mod)
    try:
        return F._load(name, path)
    finally:
        for mod in added:
            if saved[mod] is None:
                sys.modules.pop(mod, None)
            else:
                sys.modules[mod] = saved[mod]


def _stand_in(flags, crop, count, read_img, **more):
    f_lr, f_ud, f_z, f_rot, f_swap = flags
    return types.SimpleNamespace(crop_size=list(crop), num=count, train_list=list(range(count)), read_img=read_img, random_fliplr=f_lr,
                                 random_flipud=f_ud, random_flipz=f_z, random_rotation=f_rot, swap=f_swap, color_jitter=False,
                                 gauss_noise=False, elastic_trans=False, **more)


def generate():
    out = {}
    # (a) the interpolation provider
    interp = _load_with_stand_ins("reference_interp_provider", REF_INTERP)
    images = C.images_of(C.INTERP_IMAGES)
    codes, swaps = set(), set()
    for fname, flags in C.INTERP_FLAG_SETS.items():
        obj = _stand_in(flags, C.INTERP_CROP, len(C.INTERP_TRIPLETS), lambda k: tuple(images[t] for t in C.INTERP_TRIPLETS[k]))
        for seed in C.INTERP_SEEDS if fname == "all" else C.INTERP_SEEDS[:C.INTERP_OTHER_SEEDS]:
            interp.random.seed(seed)
            im, lb = interp.Train.__getitem__(obj, 0)
            key = "i_%s_%d_" % (fname, seed)
            out[key + "im"], out[key + "lb"], out[key + "next"] = im, lb, np.float64(interp.random.random())
            assert im.dtype == np.float32 and lb.dtype == np.float32 and im.shape == (6,) + C.INTERP_CROP and lb.shape == (1,) + C.INTERP_CROP
            if fname == "all":
                import random
                draw = C.draw_sample(random.Random(seed), flags, [images[t[0]].shape for t in C.INTERP_TRIPLETS], C.INTERP_CROP)
                codes.add(C.orientation_code(*draw[3]))
                swaps.add(draw[4])
    assert codes == set(range(8)) and swaps == {False, True}, "the seeds must show all eight codes and both swap outcomes: %s %s" % (codes, swaps)
    for img in images:                                     # the provider worked on copies
        assert img.flags.owndata
    assert all(np.array_equal(a, b) for a, b in zip(images, C.images_of(C.INTERP_IMAGES)))
    # (b) the fusion provider, degradation bound
    _, _, fusion = F._reference_modules()
    images = C.images_of(C.FUSION_IMAGES)
    offset = (C.FUSION_CROP[0] - C.FUSION_DET) // 2
    for seed in C.FUSION_SEEDS:
        obj = _stand_in(C.FUSION_FLAGS, C.FUSION_CROP, len(C.FUSION_PAIRS), None, interp_train_list=list(range(len(C.FUSION_PAIRS))),
                        det_size=C.FUSION_DET, offset=offset, gt_line=bool(seed & 1))
        obj.read_img = lambda a, b: (images[C.FUSION_PAIRS[a][0]], images[C.FUSION_PAIRS[b][1]])
        obj.degradation = types.MethodType(fusion.Train.degradation, obj)
        fusion.random.seed(seed)
        im, lb = fusion.Train.__getitem__(obj, 0)
        key = "f_%d_" % seed
        out[key + "im"], out[key + "lb"], out[key + "next"] = im, lb, np.float64(fusion.random.random())
        assert im.dtype == np.float32 and lb.dtype == np.float32 and im.shape == (6, C.FUSION_DET, C.FUSION_DET) and lb.shape == (1, C.FUSION_DET, C.FUSION_DET)
    # (c) the SP loops' RotationFlip
    sp = _load_with_stand_ins("reference_sp_dataset", REF_SP, always=("utils", "utils.util"))
    square = C.image(*C.SP_SQUARE)
    out["sp_case"] = np.stack([np.ascontiguousarray(sp.ImageDataset.RotationFlip(None, square, case)) for case in range(8)])
    assert len({a.tobytes() for a in out["sp_case"]}) == 8
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "crop_batch.npz")
    data = generate()
    np.savez_compressed(path, **data)
    print("arrays:", len(data))
    print("wrote", path, os.path.getsize(path), "bytes; fold.npz is", os.path.getsize(os.path.join(HERE, "fold.npz")))
