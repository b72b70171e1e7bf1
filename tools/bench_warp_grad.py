#!/usr/bin/env python
"""Developer benchmark: the back-warp's two gradient launches (sstem_warp_bilinear_backward_f32: the flow gradient, and the clear +
atomic image gradient), each next to a pure stream (one device copy) of the bytes the launch moves, and next to a plain-torch
restatement of the reference module (sff_scripts_fusion/utils/image_warp_torch.py: pad, floor, clamp, four gathers, weighted sum)
differentiated by autograd, at the fusion loop's batch [16,3,256,256] and an inference-sized [8,3,1024,1024].

Byte model per pixel of B*H*W (fp32): flow gradient 2 (flow) + C (grad_output) + 4 C (taps; neighbours share cache lines, so HBM sees
about C) + 2 (store) -> counted as (4 + 2 C) dwords; image gradient 2 + C read, C cleared, 4 C atomic dwords -> (2 + 6 C) dwords.

The paths ALTERNATE inside one process after a warm-up: ``--windows`` windows per path, each of ``--iters`` calls between two device
events; the spread is the sample standard deviation of a path's window means.  One JSON line per shape and kind of flow
(``--flows``: "smooth" = +-4 px varying over ~32 px, as a flow net's output; "noise" = +-4 px independently per pixel, the scatter's
worst case).

    timeout 300 python tools/bench_warp_grad.py
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "sstem-restoration_amd"))

import sstem_native  # noqa: E402


def _prewarm(seconds):
    """An idle MI355X needs a few hundred ms under load to reach its clocks."""
    a = torch.randn(4096, 4096, device="cuda")
    t0 = time.time()
    while time.time() - t0 < seconds:
        (a @ a).sum().item()


def _window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3        # us per call


def warp_torch(img, flow):
    """The reference module's arithmetic in plain torch, NCHW (img [B,C,H,W], flow [B,2,H,W])."""
    B, C, H, W = img.shape
    P = F.pad(img, (1, 1, 1, 1)).reshape(B, C, -1)
    x = flow[:, 0] + torch.arange(W, device=img.device, dtype=torch.float32) + 1
    y = flow[:, 1] + torch.arange(H, device=img.device, dtype=torch.float32)[:, None] + 1
    x0 = torch.floor(x).long(); y0 = torch.floor(y).long()
    x1 = torch.clamp(x0 + 1, 0, W + 1); y1 = torch.clamp(y0 + 1, 0, H + 1)
    x0 = torch.clamp(x0, 0, W + 1); y0 = torch.clamp(y0, 0, H + 1)
    wx = (x1.float() - x)[:, None]; wy = (y1.float() - y)[:, None]

    def tap(yy, xx):
        return P.gather(2, (yy * (W + 2) + xx).view(B, 1, -1).expand(B, C, -1)).view(B, C, H, W)
    return wx * wy * tap(y0, x0) + wx * (1 - wy) * tap(y1, x0) + (1 - wx) * wy * tap(y0, x1) + (1 - wx) * (1 - wy) * tap(y1, x1)


def _kernels(a):
    lib = sstem_native.load_library()
    stream = torch.cuda.current_stream().cuda_stream
    for shape, kind in ((s, k) for s in a.shapes.split(",") for k in a.flows.split(",")):
        B, C, H, W = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda"); g.manual_seed(17)
        img = torch.rand(B, C, H, W, device="cuda", generator=g)
        if kind == "smooth":          # +-4 px varying over ~32 px, as a flow net's output does: neighbouring lanes hit neighbouring addresses
            flow = F.interpolate((torch.rand(B, 2, H // 32 + 2, W // 32 + 2, device="cuda", generator=g) - 0.5) * 8.0, size=(H, W),
                                 mode="bilinear", align_corners=True).contiguous()
        else:                         # "noise": +-4 px independently per pixel -- every lane of a wave scatters to an address of its own
            flow = (torch.rand(B, 2, H, W, device="cuda", generator=g) - 0.5) * 8.0
        gout = torch.randn(B, C, H, W, device="cuda", generator=g)
        gf, gi = torch.empty_like(flow), torch.empty_like(img)

        def entry(want_flow, want_img):
            rc = lib.sstem_warp_bilinear_backward_f32(img.data_ptr() if want_flow else None, flow.data_ptr(), gout.data_ptr(),
                                                      gf.data_ptr() if want_flow else None, gi.data_ptr() if want_img else None, 0,
                                                      B, C, H, W, stream)
            sstem_native.check(rc, "sstem_warp_bilinear_backward_f32")
        dwords = {"flow": (4 + 2 * C) * B * H * W, "image": (2 + 6 * C) * B * H * W}
        src = {k: torch.empty(n // 2, device="cuda") for k, n in dwords.items()}        # a copy reads and writes each element
        dst = {k: torch.empty_like(v) for k, v in src.items()}
        leaf_i, leaf_f = img.clone().requires_grad_(True), flow.clone().requires_grad_(True)
        out_f = warp_torch(img, leaf_f)
        out_i = warp_torch(leaf_i, flow)
        paths = {
            "flow_grad": lambda: entry(True, False),
            "flow_stream": lambda: dst["flow"].copy_(src["flow"]),
            "flow_torch_backward": lambda: torch.autograd.grad(out_f, leaf_f, gout, retain_graph=True),
            "flow_torch_forward_backward": lambda: torch.autograd.grad(warp_torch(img, leaf_f), leaf_f, gout),
            "image_grad": lambda: entry(False, True),
            "image_stream": lambda: dst["image"].copy_(src["image"]),
            "image_torch_backward": lambda: torch.autograd.grad(out_i, leaf_i, gout, retain_graph=True),
            "both_grads": lambda: entry(True, True),
        }
        for _ in range(5):
            for fn in paths.values():
                fn()
        torch.cuda.synchronize()
        entry(True, True); torch.cuda.synchronize()
        t_f, = torch.autograd.grad(out_f, leaf_f, gout, retain_graph=True)
        t_i, = torch.autograd.grad(out_i, leaf_i, gout, retain_graph=True)
        times = {k: [] for k in paths}
        for _ in range(a.windows):
            for k, fn in paths.items():
                times[k].append(_window(fn, a.iters))
        row = {"shape": [B, C, H, W], "flow": kind, "windows": a.windows, "iters": a.iters,
               "flow_bytes": 4 * dwords["flow"], "image_bytes": 4 * dwords["image"],
               "flow_grad_rel_diff_vs_torch": float((gf - t_f).abs().max() / t_f.abs().max()),
               "image_grad_rel_diff_vs_torch": float((gi - t_i).abs().max() / t_i.abs().max())}
        for k, v in times.items():
            row[k + "_us"] = round(statistics.mean(v), 2)
            row[k + "_spread_us"] = round(statistics.stdev(v), 2) if len(v) > 1 else 0.0
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16x3x256x256,8x3x1024x1024")
    ap.add_argument("--flows", default="smooth,noise")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_warp_grad needs a GPU")
    _prewarm(0.8)
    _kernels(a)


if __name__ == "__main__":
    main()
