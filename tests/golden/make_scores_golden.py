"""Generates tests/golden/scores.npz from the REFERENCE's compute_psnr / compute_ssim (utils/psnr_ssim.py) and EPE
(loss/multiscaleloss.py), imported in place from the reference tree (nothing is copied), on the CPU.

One intervention: psnr_ssim.py imports ``skimage.io`` at its top and skimage is not installed here, so an empty stand-in module is
registered under that name while the file is imported; the scored functions never touch it when they are given arrays.

Per image case ``<name>`` (tests/scores_ref64.py: IMAGE_CASES, make_image_case) the file holds the two images, the reference's
``mse`` (NaN where it returns its bare sentinel and no mse), ``psnr`` (1e12 there) and ``ssim``, and how far each is from the float64
restatement: ``dev_mse`` (relative), ``dev_psnr`` (absolute, dB), ``dev_ssim`` (absolute).  Per flow case (FLOW_CASES, make_flow_case)
the two flows, ``epe[sparse][mean]`` as the reference's float32 results and ``dev_epe[sparse][mean]`` (relative; 0 where both are NaN).

    python tests/golden/make_scores_golden.py [out.npz]
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import scores_ref64 as R  # noqa: E402

REF = os.environ.get("SSTEM_REFERENCE", "/root/reference")
REF_SCORES = os.path.join(REF, "sff_scripts_unfolding", "utils", "psnr_ssim.py")
REF_EPE = os.path.join(REF, "sff_scripts_unfolding", "loss", "multiscaleloss.py")


def reference_available():
    return os.path.exists(REF_SCORES) and os.path.exists(REF_EPE)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _reference_modules():
    added = [n for n in ("skimage", "skimage.io") if n not in sys.modules]
    if added:
        pkg = types.ModuleType("skimage")
        pkg.io = types.ModuleType("skimage.io")
        sys.modules["skimage"], sys.modules["skimage.io"] = pkg, pkg.io
    try:
        return _load("reference_psnr_ssim", REF_SCORES), _load("reference_multiscaleloss", REF_EPE)
    finally:
        for n in added:
            sys.modules.pop(n, None)


def generate():
    torch.set_num_threads(1)             # one summation order, whatever machine regenerates the file
    scores, epe = _reference_modules()
    out = {}
    for name in R.IMAGE_CASES:
        a, b = R.make_image_case(name)
        got = scores.compute_psnr(a, b)
        mse, psnr = (np.nan, 1.0e12) if not isinstance(got, tuple) and got == R.SENTINEL else got
        ssim = scores.compute_ssim(a, b)
        mse64, psnr64 = R.psnr64(torch.from_numpy(a), torch.from_numpy(b))
        ssim64 = R.ssim64(torch.from_numpy(a), torch.from_numpy(b))
        k = name + "_"
        out[k + "a"], out[k + "b"] = a, b
        out[k + "mse"], out[k + "psnr"], out[k + "ssim"] = np.float64(mse), np.float64(psnr), np.float64(ssim)
        out[k + "dev_mse"] = np.float64(0.0 if np.isnan(mse) else abs(float(mse) - mse64) / mse64)
        out[k + "dev_psnr"] = np.float64(abs(float(psnr) - psnr64))
        out[k + "dev_ssim"] = np.float64(abs(float(ssim) - ssim64))
    for name in R.FLOW_CASES:
        flow, target = R.make_flow_case(name)
        f, t = torch.from_numpy(flow), torch.from_numpy(target)
        got = np.zeros((2, 2), dtype=np.float32)
        dev = np.zeros((2, 2), dtype=np.float64)
        for sparse in (0, 1):
            for mean in (0, 1):
                v = epe.EPE(f, t, sparse=bool(sparse), mean=bool(mean))
                assert v.dtype == torch.float32
                got[sparse, mean] = float(v)
                v64 = R.epe64(f, t, bool(sparse), bool(mean))
                if np.isnan(v64) and np.isnan(got[sparse, mean]):
                    dev[sparse, mean] = 0.0
                else:
                    dev[sparse, mean] = abs(float(got[sparse, mean]) - v64) / abs(v64) if v64 != 0 else abs(float(got[sparse, mean]))
        k = name + "_"
        out[k + "flow"], out[k + "target"], out[k + "epe"], out[k + "dev_epe"] = flow, target, got, dev
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "scores.npz")
    data = generate()
    np.savez_compressed(path, **data)
    for name in R.IMAGE_CASES:
        k = name + "_"
        print("%-8s mse %.6e psnr %.6f ssim %.9f  dev mse %.2e psnr %.2e ssim %.2e"
              % (name, data[k + "mse"], data[k + "psnr"], data[k + "ssim"], data[k + "dev_mse"], data[k + "dev_psnr"], data[k + "dev_ssim"]))
    for name in R.FLOW_CASES:
        k = name + "_"
        print("%-12s epe %s dev %s" % (name, data[k + "epe"].ravel(), data[k + "dev_epe"].ravel()))
    print("wrote", path, os.path.getsize(path), "bytes")
