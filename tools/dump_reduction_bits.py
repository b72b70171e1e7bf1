#!/usr/bin/env python
"""Developer check for changes to the launch-wide reductions (csrc/wg_reduce.h) and to the SSIM blurs of the kernels on it: from fixed seeds,
every output of the MS-SSIM criterion, the validation scores, the flow EPE and the fused L1 loss at the smallest shapes that reach each
branch of the shared code, into one ``.npz``.  Every call is made twice on one workspace and both results are kept (``.../run0``,
``.../run1``): the second equals the first when the last workgroup's counter reset works.

    python tools/dump_reduction_bits.py --out before.npz          # at the commit to compare against (copy this file there)
    python tools/dump_reduction_bits.py --out after.npz
    python tools/dump_reduction_bits.py --compare before.npz after.npz

``--compare`` needs no GPU: array by array, dtype, shape and raw bytes (so NaNs compare by their bits); exit status 1 on any difference.
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "sstem-restoration_amd"))


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.frombuffer(a.tobytes(), np.uint8), np.frombuffer(b.tobytes(), np.uint8))


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in bad:
        print("only in one file: %s" % k)
    for k in sorted(set(a.files) & set(b.files)):
        ok = same_bits(a[k], b[k])
        print("%-9s %s %s%s" % ("equal" if ok else "DIFFERENT", k, a[k].dtype, list(a[k].shape)))
        if not ok:
            bad.append(k)
    print("%d arrays, %d different" % (len(set(a.files) | set(b.files)), len(bad)))
    return 1 if bad else 0


def dump(out_path):
    import torch
    import train_utils
    from loss.loss_ssim import MS_SSIM
    from loss.multiscaleloss import _epe_float64
    from utils.psnr_ssim import score_batch

    if not torch.cuda.is_available():
        raise SystemExit("dump_reduction_bits needs a GPU")
    dev = torch.device("cuda:0")
    out = {}

    def keep(name, run, **tensors):
        for k, t in tensors.items():
            out["%s/%s/run%d" % (name, k, run)] = t.detach().cpu().numpy()

    def gpu(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    # MS-SSIM: value, per-level terms, gradient for both images
    for (B, H, W), levels in (((3, 33, 33), 3), ((2, 70, 45), 2), ((1, 9, 40), 1), ((5, 230, 250), 1)):
        rng = np.random.default_rng(1000 + H)
        x = rng.random((B, 1, H, W), dtype=np.float32)
        y = np.clip(x + 0.1 * rng.standard_normal((B, 1, H, W), dtype=np.float32), 0, 1).astype(np.float32)
        crit = MS_SSIM(max_val=1.0)
        for run in range(2):
            a, b = gpu(x).requires_grad_(), gpu(y).requires_grad_()
            _, terms = crit.level_terms(a, b, levels)
            value = crit.ms_ssim(a, b, levels)
            value.backward()
            keep("ms_ssim_%dx%dx%d_L%d" % (B, H, W, levels), run, value=value, terms=terms, grad1=a.grad, grad2=b.grad)

    # scores: (mse, psnr, ssim) per image
    def unit(rng, shape):
        a = rng.random(shape, dtype=np.float32)
        return a, np.clip(a + 0.05 * rng.standard_normal(shape, dtype=np.float32), 0, 1).astype(np.float32)

    rng = np.random.default_rng(2000)
    cases = {}
    cases["f32_3x43x44_unit"] = unit(rng, (3, 43, 44)) + (False,)
    u = rng.integers(0, 256, (2, 75, 53), dtype=np.uint8)
    cases["u8_2x75x53"] = (u, np.clip(u.astype(np.int32) + rng.integers(-9, 10, u.shape), 0, 255).astype(np.uint8), False)
    a, b = unit(rng, (2, 70, 130))
    cases["f32_2x70x130_255"] = (a * 255, b * 255, False)
    cases["f32_2x154x266_unit"] = unit(rng, (2, 154, 266)) + (False,)
    a, b = unit(rng, (3, 43, 44))
    cases["f32_3x43x44_clamp01"] = ((a * 1.4 - 0.2).astype(np.float32), b, True)
    a, b = unit(rng, (3, 43, 44))
    a[1, 20, 7] = np.nan
    cases["f32_3x43x44_nan_in_image1"] = (a, b, False)
    for name, (a, b, clamp01) in cases.items():
        ta, tb = gpu(a), gpu(b)
        for run in range(2):
            keep("scores_" + name, run, scores=score_batch(ta, tb, clamp01=clamp01))

    # flow EPE, sparse x mean
    for B, H, W in ((2, 37, 29), (2, 520, 520)):
        rng = np.random.default_rng(3000 + H)
        target = rng.standard_normal((B, 2, H, W), dtype=np.float32)
        target[np.broadcast_to(rng.random((B, 1, H, W)) < 1 / 3, target.shape)] = 0
        flow = target + 0.5 * rng.standard_normal((B, 2, H, W), dtype=np.float32)
        tf, tt = gpu(flow), gpu(target)
        for sparse in (False, True):
            for mean in (False, True):
                for run in range(2):
                    keep("epe_%dx%dx%d_sparse%d_mean%d" % (B, H, W, sparse, mean), run, value=_epe_float64(tf, tt, sparse, mean))

    # fused L1: loss and gradient; n = 4099 on views one float past an aligned address (the scalar path)
    for n, offset in ((5, 0), (4099, 1), (1024 * 1024 + 3, 0)):
        rng = np.random.default_rng(4000 + n)
        p, t = rng.standard_normal(n + offset, dtype=np.float32), rng.standard_normal(n + offset, dtype=np.float32)
        t[::7] = p[::7]
        tp, tt = gpu(p)[offset:], gpu(t)[offset:]
        crit = train_utils.L1MeanLoss(dev)
        for run in range(2):
            loss, grad = crit(tp, tt)
            keep("l1_n%d_offset%d" % (n, offset), run, loss=loss, grad=grad)

    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez(out_path, **out)
    unstable = [k for k in out if k.endswith("/run0") and not same_bits(out[k], out[k[:-1] + "1"])]
    for k in unstable:
        print("second call differs from the first: %s" % k[:-5])
    print("%d arrays -> %s; second call equals first: %s" % (len(out), out_path, "no" if unstable else "yes"))
    return 1 if unstable else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="reduction_bits.npz")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    sys.exit(compare(*a.compare) if a.compare else dump(a.out))


if __name__ == "__main__":
    main()
