"""Generates tests/golden/ms_ssim.npz from the REFERENCE's MS_SSIM class, imported in place from the reference tree (nothing is
copied), on the CPU.

One intervention: ``torch.Tensor.cuda`` is patched to return ``self`` while the reference runs, because its module calls ``.cuda()`` on
the window and on the level weights (loss_ssim.py:29,52-55); the arithmetic is untouched.

Per case ``c<i>`` (tests/ms_ssim_ref64.py: CASES, make_pair) the file holds the inputs, the reference's fp32 value, its fp32 autograd
gradient with respect to img1 and the per-level terms, and how far each of those is from the float64 restatement ``ref64``:
``*_dev_value`` (absolute), ``*_dev_terms`` (largest absolute over the levels' two terms), ``*_dev_grad`` (max-norm relative to the
gradient's max).  The GPU tests derive their bounds from these deviations.

    python tests/golden/make_ms_ssim_golden.py [out.npz]
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ms_ssim_ref64 as R  # noqa: E402

REF = os.environ.get("SSTEM_REFERENCE", "/root/reference")
REF_FILE = os.path.join(REF, "sff_scripts_fusion", "loss", "loss_ssim.py")


def reference_available():
    return os.path.exists(REF_FILE)


def _reference_module():
    spec = importlib.util.spec_from_file_location("reference_loss_ssim", REF_FILE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _reference_run(mod, pred, target, max_val):
    """The reference's forward, its per-level means (a second pass through its own _ssim) and its autograd gradient, fp32 on the CPU."""
    crit = mod.MS_SSIM(max_val=max_val)
    a = torch.from_numpy(pred).requires_grad_(True)
    b = torch.from_numpy(target)
    value = crit(a, b)
    value.backward()
    terms = []
    with torch.no_grad():
        x, y = a.detach(), b
        for _ in range(5):
            s, m = crit._ssim(x, y)
            terms.append((float(s), float(m)))
            x, y = torch.nn.functional.avg_pool2d(x, 2, 2), torch.nn.functional.avg_pool2d(y, 2, 2)
    return np.float32(value.item()), np.asarray(terms, dtype=np.float32), a.grad.numpy().copy()


def generate():
    torch.set_num_threads(1)             # one summation order, whatever machine regenerates the file
    mod = _reference_module()
    out = {}
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        for i, ((B, H, W), max_val) in enumerate(R.CASES):
            pred, target = R.make_pair(B, H, W, R.case_seed(i), scale=max_val)
            value, terms, grad = _reference_run(mod, pred, target, max_val)
            v64, t64, g64 = R.ref64(torch.from_numpy(pred), torch.from_numpy(target), max_val, 5)
            g64 = g64.numpy()
            k = "c%d_" % i
            out[k + "pred"], out[k + "target"] = pred, target
            out[k + "max_val"] = np.float32(max_val)
            out[k + "value"], out[k + "terms"], out[k + "grad"] = value, terms, grad
            out[k + "dev_value"] = np.float64(abs(float(value) - float(v64)))
            out[k + "dev_terms"] = np.float64(np.abs(terms.astype(np.float64) - t64.numpy()).max())
            out[k + "dev_grad"] = np.float64(np.abs(grad.astype(np.float64) - g64).max() / np.abs(g64).max())
    finally:
        torch.Tensor.cuda = real_cuda
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ms_ssim.npz")
    data = generate()
    np.savez_compressed(path, **data)
    for i in range(len(R.CASES)):
        k = "c%d_" % i
        print(R.CASES[i], "value %.7f" % data[k + "value"], "mcs", np.round(data[k + "terms"][:, 1], 4),
              "dev value %.2e terms %.2e grad %.2e" % (data[k + "dev_value"], data[k + "dev_terms"], data[k + "dev_grad"]))
    print("wrote", path, os.path.getsize(path), "bytes")
