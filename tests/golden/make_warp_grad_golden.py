"""Generates tests/golden/warp_grad.npz: the REFERENCE module ``sff_scripts_fusion/utils/image_warp_torch.py`` (pure torch) run on
the CPU in fp32 with BOTH inputs requiring a gradient -- the gradients torch's autograd derives from it, which
sstem_warp_bilinear_backward_f32 computes natively.  Per case: ``_img`` [B,C,H,W], ``_flow`` [B,2,H,W], ``_g`` = dL/dout, and the
recorded ``_grad_flow`` [B,2,H,W], ``_grad_img``, ``_out``.

    python tests/golden/make_warp_grad_golden.py REFERENCE_ROOT

Every case keeps B*H*W >= 2: the reference's ``torch.squeeze`` (:93) would drop a pixel axis of length one."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import warp_grad_ref64 as R  # noqa: E402

CASES = ("rand", "knots", "zero", "sides", "p1x1", "c1", "many")


def _to(targets, n):
    """A flow plane that sends index i (0-based) to the PADDED coordinate targets[i]: x = (flow + i) + 1."""
    return np.asarray(targets, np.float32) - np.arange(n, dtype=np.float32) - np.float32(1)


def inputs():
    rng = np.random.default_rng(20240607)
    c = {}

    def put(name, img_shape, flow):
        c[name] = (rng.random(img_shape, dtype=np.float32), np.ascontiguousarray(flow, np.float32),
                   rng.standard_normal(img_shape).astype(np.float32))

    put("rand", (2, 3, 9, 13), rng.uniform(-4, 4, (2, 2, 9, 13)))
    f = np.round(rng.uniform(-3, 3, (1, 2, 6, 8)))
    f[:, :, 3:] += 0.5                                         # rows 0-2 integer knots, rows 3-5 half-integer
    f[:, 1, :, ::2] = np.round(f[:, 1, :, ::2])                # ... and mixed: integer in y, half-integer in x
    put("knots", (1, 2, 6, 8), f)
    put("zero", (1, 2, 4, 4), np.zeros((1, 2, 4, 4)))
    H, W = 9, 10
    f = np.zeros((2, 2, H, W), np.float32)
    # sample 0: row r lands on the padded x of xs[r] (off the left, exactly 0, 1, W, W+1, off the right), y a quarter pixel down
    xs = [-1.5, 0, 0.25, 1, W, W + 0.5, W + 1, W + 2.5, 3.75]
    f[0, 0] = np.stack([_to([v] * W, W) for v in xs]); f[0, 1] = 0.25
    # sample 1: column c lands on the padded y of ys[c] (off the top, exactly 0, 1, H, H+1, off the bottom), x half a pixel left
    ys = [-1.5, 0, 0.5, 1, H, H + 0.75, H + 1, H + 3, 2.25, -40]
    f[1, 1] = np.stack([_to([v] * H, H) for v in ys], 1); f[1, 0] = -0.5
    put("sides", (2, 2, H, W), f)
    put("p1x1", (2, 2, 1, 1), np.array([[[[0.25]], [[-0.5]]], [[[0.0]], [[0.0]]]]))
    put("c1", (2, 1, 5, 7), rng.uniform(-2, 2, (2, 2, 5, 7)))
    put("many", (1, 2, 5, 7), R.many_to_one_flow(1, 5, 7, 2.25, 3.5))
    assert tuple(c) == CASES
    return c


def main(reference_root):
    spec = importlib.util.spec_from_file_location("ref_warp", os.path.join(reference_root, "sff_scripts_fusion", "utils", "image_warp_torch.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    warp = ref.SpatialTransformation(use_gpu=False)
    out = {}
    for name, (img, flow, g) in inputs().items():
        ti = torch.from_numpy(img).requires_grad_(True)
        tf = torch.from_numpy(flow).requires_grad_(True)
        res = warp(ti, tf.permute(0, 2, 3, 1))
        assert res.shape == ti.shape and res.dtype == torch.float32
        res.backward(torch.from_numpy(g))
        r = R.ref64(img, flow, g)
        print("%-6s %-14s |grad_flow - ref64| max %.2e (max |grad| %.2f)   |grad_img - ref64| max %.2e" % (
            name, img.shape, np.abs(tf.grad.numpy() - r["grad_flow"]).max(), np.abs(r["grad_flow"]).max(),
            np.abs(ti.grad.numpy() - r["grad_image"]).max()))
        out[name + "_img"], out[name + "_flow"], out[name + "_g"] = img, flow, g
        out[name + "_out"] = res.detach().numpy()
        out[name + "_grad_flow"], out[name + "_grad_img"] = tf.grad.numpy(), ti.grad.numpy()
    path = os.path.join(HERE, "warp_grad.npz")
    np.savez_compressed(path, **out)
    print("wrote warp_grad.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
