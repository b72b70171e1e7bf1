"""Generates tests/golden/ssim_loss.npz from the REFERENCE's single-scale SSIMLoss, imported in place from the reference tree (nothing
is copied), on the CPU.  No intervention is needed: sff_scripts_interp/loss/loss_ssim.py:74-146 runs on CPU tensors as it stands.

Per case ``c<i>`` (tests/ssim_loss_ref64.py: CASES, make_case) the file holds the inputs, the reference's fp32 value
(``SSIMLoss(size_average=...)(pred, target)``: a scalar, or [B]) and its fp32 autograd gradient of the value's sum with respect to
img1, and how far each is from a float64 run of the SAME code on the same inputs (the module's window follows the images' dtype):
``*_dev_value`` (largest absolute) and ``*_dev_grad`` (max-norm relative to the gradient's max).  The GPU tests derive their bounds
from these deviations.

    python tests/golden/make_ssim_loss_golden.py [out.npz]
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ssim_loss_ref64 as R  # noqa: E402

REF = os.environ.get("SSTEM_REFERENCE", "/root/reference")
REF_FILE = os.path.join(REF, "sff_scripts_interp", "loss", "loss_ssim.py")


def reference_available():
    return os.path.exists(REF_FILE)


def _reference_module():
    spec = importlib.util.spec_from_file_location("reference_interp_loss_ssim", REF_FILE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _reference_run(mod, pred, target, size_average, dtype):
    a = torch.from_numpy(pred).to(dtype).requires_grad_(True)
    b = torch.from_numpy(target).to(dtype)
    value = mod.SSIMLoss(size_average=size_average)(a, b)
    value.sum().backward()
    return value.detach().numpy().copy(), a.grad.numpy().copy()


def generate():
    torch.set_num_threads(1)             # one summation order, whatever machine regenerates the file
    mod = _reference_module()
    out = {}
    for i, (shape, size_average) in enumerate(R.CASES):
        pred, target = R.make_case(i)
        value, grad = _reference_run(mod, pred, target, size_average, torch.float32)
        v64, g64 = _reference_run(mod, pred, target, size_average, torch.float64)
        assert value.dtype == np.float32 and grad.dtype == np.float32 and np.isfinite(value).all() and np.isfinite(grad).all()
        k = "c%d_" % i
        out[k + "pred"], out[k + "target"] = pred, target
        out[k + "size_average"] = np.bool_(size_average)
        out[k + "value"], out[k + "grad"] = value, grad
        out[k + "dev_value"] = np.float64(np.abs(value.astype(np.float64) - v64).max())
        out[k + "dev_grad"] = np.float64(np.abs(grad.astype(np.float64) - g64).max() / np.abs(g64).max())
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ssim_loss.npz")
    data = generate()
    np.savez_compressed(path, **data)
    for i in range(len(R.CASES)):
        k = "c%d_" % i
        print(R.CASES[i], "value", np.round(data[k + "value"], 6), "dev value %.2e grad %.2e" % (data[k + "dev_value"], data[k + "dev_grad"]))
    print("wrote", path, os.path.getsize(path), "bytes")
