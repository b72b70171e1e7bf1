"""Generates tests/golden/fold.npz from the REFERENCE's gen_flow (utils/flow_synthesis.py), image_warp (utils/image_warp.py) and
Train.degradation (data/data_provider.py) of sff_scripts_fusion, imported in place from the reference tree (nothing is copied), on the CPU.

Interventions: data_provider.py imports cv2, h5py, torchvision and tifffile at its top, which are not installed here (and, by an old
path, scipy.ndimage.interpolation / .filters); whichever of its imports fails is registered as an empty stand-in module while the file
is imported -- degradation touches none of them.  Its own ``utils.*`` imports are bound to the reference's files for that moment too.
Train.degradation runs unbound on a stand-in object that carries only what it reads: ``crop_size`` and ``offset``.

The file holds, with the cases and the seeded images of tests/fold_ref.py (the images are not stored):
  (a) per fold ``<name>``: ``_row`` the fold's doubles as this machine derived them (fold_ref.scalars), the reference's ``_flow``,
      ``_flow2`` (float32 [H,W,2]), ``_mask`` (uint8), ``_warp_bilinear`` and ``_warp_nearest`` (image_warp of the case's image) and
      ``_deformed`` = (warp_bilinear * mask).astype(np.uint8);
  (b) per seed ``s<seed>``: ``_deformed`` and ``_flow2`` ([h,w,2]) that degradation returned after random.seed(seed), and ``_drawn``,
      the number of candidate folds it drew (counted through a wrapper around gen_flow).

    python tests/golden/make_fold_golden.py [out.npz]
"""
import importlib
import importlib.util
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import fold_ref as R  # noqa: E402

REF = os.environ.get("SSTEM_REFERENCE", "/root/reference")
REF_DIR = os.path.join(REF, "sff_scripts_fusion")
REF_FLOW = os.path.join(REF_DIR, "utils", "flow_synthesis.py")
REF_WARP = os.path.join(REF_DIR, "utils", "image_warp.py")
REF_PROVIDER = os.path.join(REF_DIR, "data", "data_provider.py")


def reference_available():
    return all(os.path.exists(p) for p in (REF_FLOW, REF_WARP, REF_PROVIDER))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Stub(types.ModuleType):
    """An empty stand-in: any attribute is another stand-in, calling one gives None."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Stub(self.__name__ + "." + name)

    def __call__(self, *a, **k):
        return None


def _reference_modules():
    flow_mod, warp_mod = _load("reference_flow_synthesis", REF_FLOW), _load("reference_image_warp", REF_WARP)
    saved = {n: sys.modules.get(n) for n in list(sys.modules) if n == "utils" or n.startswith("utils.")}
    added = []

    def register(name, mod):
        if name not in saved:
            saved[name] = sys.modules.get(name)
        sys.modules[name] = mod
        added.append(name)

    pkg = types.ModuleType("utils")
    pkg.__path__ = []
    pkg.flow_synthesis, pkg.image_warp, pkg.flow_display = flow_mod, warp_mod, _Stub("utils.flow_display")
    register("utils", pkg)
    register("utils.flow_synthesis", flow_mod)
    register("utils.image_warp", warp_mod)
    register("utils.flow_display", pkg.flow_display)
    for name in ("cv2", "h5py", "torchvision", "tifffile", "joblib", "scipy.ndimage.interpolation", "scipy.ndimage.filters"):
        try:
            importlib.import_module(name)
        except Exception:
            register(name, _Stub(name))
    try:
        provider = _load("reference_data_provider", REF_PROVIDER)
    finally:
        for name in added:
            if saved.get(name) is None:
                sys.modules.pop(name, None)
            else:
                sys.modules[name] = saved[name]
    return flow_mod, warp_mod, provider


def generate():
    flow_mod, warp_mod, provider = _reference_modules()
    out = {}
    for name in R.FOLD_CASES:
        H, W, (k, b, lw, fw, dis_k), img = R.fold_case(name)
        flow, flow2, mask = flow_mod.gen_flow(H, W, k, b, lw, fw, dis_k)
        assert flow.dtype == np.float32 and flow2.dtype == np.float32 and mask.dtype == np.float64
        bil = warp_mod.image_warp(img, flow, mode="bilinear")
        near = warp_mod.image_warp(img, flow, mode="nearest")
        key = name + "_"
        out[key + "row"] = R.scalars(k, b, lw, fw, dis_k)
        out[key + "flow"], out[key + "flow2"], out[key + "mask"] = flow, flow2, mask.astype(np.uint8)
        out[key + "warp_bilinear"], out[key + "warp_nearest"] = bil, near
        out[key + "deformed"] = (bil * mask).astype(np.uint8)
    # (b) the rejection loop: gen_flow counted through the name data_provider.py bound at its import
    calls = [0]
    gen_flow = provider.gen_flow

    def counted(*a, **kw):
        calls[0] += 1
        return gen_flow(*a, **kw)

    provider.gen_flow = counted
    stand_in = types.SimpleNamespace(crop_size=[R.DEGRADE_SIZE, R.DEGRADE_SIZE], offset=R.DEGRADE_OFFSET)
    clean = R.image(R.DEGRADE_IMAGE_SEED, R.DEGRADE_SIZE, R.DEGRADE_SIZE)
    drawn = []
    for seed in R.DEGRADE_SEEDS:
        calls[0] = 0
        provider.random.seed(seed)
        deformed, flow2 = provider.Train.degradation(stand_in, clean)
        key = "s%d_" % seed
        out[key + "deformed"], out[key + "flow2"], out[key + "drawn"] = deformed, np.ascontiguousarray(flow2), np.int64(calls[0])
        drawn.append(calls[0])
    assert any(d > 1 for d in drawn) and any(d == 1 for d in drawn), "the seeds must show a rejection and a first-draw acceptance: %s" % drawn
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "fold.npz")
    data = generate()
    np.savez_compressed(path, **data)
    for name in R.FOLD_CASES:
        f = data[name + "_flow"]
        print("%-12s %s  -0.0 in flow: %d  black: %d" % (name, f.shape[:2], int((np.signbit(f) & (f == 0)).sum()), int((data[name + "_deformed"] == 0).sum())))
    print("candidates drawn per seed:", [int(data["s%d_drawn" % s]) for s in R.DEGRADE_SEEDS])
    print("wrote", path, os.path.getsize(path), "bytes")
