#!/usr/bin/env python
"""Developer benchmark: the validation scores as launches (utils.psnr_ssim.score_batch: mse, PSNR and SSIM per image, two launches;
loss.multiscaleloss.EPE: one launch) against what the reference does -- copy the tensors to the host and score them there in
float64 (tests/scores_ref64.py, the restatement of its numpy / scipy formulation on torch).

The native path is timed between two device events, ``--windows`` windows of ``--iters`` calls after a warm-up; the host path
(device -> host copy + scoring, which synchronises by itself) by the wall clock, ``--host-windows`` windows of ``--host-iters`` calls.
The spread reported is the sample standard deviation of a path's window means.  Prints one JSON line per shape.

    timeout 600 python tools/bench_scores.py
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "sstem-restoration_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import scores_ref64 as R  # noqa: E402
from loss.multiscaleloss import EPE  # noqa: E402
from utils.psnr_ssim import score_batch  # noqa: E402


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


def _host_window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    return (time.perf_counter() - t0) / iters * 1e6


def _row(what, shape, native, host, a):
    for _ in range(20):
        native()
    host()
    torch.cuda.synchronize()
    tn = [_window(native, a.iters) for _ in range(a.windows)]
    th = [_host_window(host, a.host_iters) for _ in range(a.host_windows)]
    return {"what": what, "shape": list(shape), "native_us": round(statistics.mean(tn), 2), "native_spread_us": round(statistics.stdev(tn), 2),
            "host_us": round(statistics.mean(th), 1), "host_spread_us": round(statistics.stdev(th), 1),
            "speedup": round(statistics.mean(th) / statistics.mean(tn), 1), "windows": a.windows, "iters": a.iters,
            "host_windows": a.host_windows, "host_iters": a.host_iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--image-shapes", default="1x1024x1024,16x256x256")
    ap.add_argument("--flow-shapes", default="16x256x256")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--host-iters", type=int, default=2)
    ap.add_argument("--host-windows", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scores needs a GPU")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    _prewarm(0.8)
    for shape in a.image_shapes.split(","):
        B, H, W = (int(v) for v in shape.split("x"))
        pairs = [R.make_pair(H, W, 17 + i) for i in range(B)]
        pred = torch.stack([torch.from_numpy(p[0]) for p in pairs]).cuda()[:, None]
        gt = torch.stack([torch.from_numpy(p[1]) for p in pairs]).cuda()[:, None]
        row = _row("score_batch", (B, 1, H, W), lambda: score_batch(pred, gt, clamp01=True),
                   lambda: R.score64(pred[:, 0].cpu(), gt[:, 0].cpu(), clamp01=True), a)
        got, want = score_batch(pred, gt, clamp01=True).cpu(), R.score64(pred[:, 0].cpu(), gt[:, 0].cpu(), clamp01=True)
        row["ssim_abs_diff"] = float((got[:, 2] - want[:, 2]).abs().max())
        row["mse_rel_diff"] = float(((got[:, 0] - want[:, 0]).abs() / want[:, 0]).max())
        print(json.dumps(row), flush=True)
    for shape in a.flow_shapes.split(","):
        B, H, W = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda"); g.manual_seed(23)
        flow = 2 * torch.randn(B, 2, H, W, device="cuda", generator=g)
        target = flow + 0.5 * torch.randn(B, 2, H, W, device="cuda", generator=g)
        row = _row("EPE", (B, 2, H, W), lambda: EPE(flow, target), lambda: R.epe64(flow.cpu(), target.cpu()), a)
        row["rel_diff"] = abs(float(EPE(flow, target)) - R.epe64(flow.cpu(), target.cpu())) / R.epe64(flow.cpu(), target.cpu())
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
