#!/usr/bin/env python
"""Developer benchmark: the single-scale SSIM criterion's value + gradient, native (train_utils.SSIMMeanLoss: two launches) against the
plain-torch formulation under autograd (loss.loss_ssim.ssim_loss_torch, what SSTEM_NATIVE_SSIM=0 selects for the interpolation step),
at the interpolation loop's batch [8,1,256,256] and one inference tile [1,1,1024,1024]; and the L2 launch (train_utils.L2MeanLoss)
against F.mse_loss + backward on the same tensors.

The two paths ALTERNATE inside one process after a warm-up: ``--windows`` windows per path and shape, each of ``--iters`` calls between
two device events, so both see the same clocks; the spread reported is the sample standard deviation of a path's window means.
Launch counts come from torch's profiler (one extra call per path, outside the timed windows).  Prints one JSON line of times per
shape and criterion, then one of launch counts.

    timeout 300 python tools/bench_ssim_loss.py
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
sys.path.insert(0, os.path.join(REPO, "tests"))

import train_utils  # noqa: E402
from loss.loss_ssim import ssim_loss_torch  # noqa: E402
from ms_ssim_ref64 import make_pair  # noqa: E402


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


def _launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn(); torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def _compare(what, shape, native, plain, a):
    for _ in range(20):
        native(); plain()
    torch.cuda.synchronize()
    v_n, g_n = native(); v_p, g_p = plain()
    agree = float((g_n - g_p).abs().max() / g_p.abs().max())
    tn, tp = [], []
    for _ in range(a.windows):
        tn.append(_window(native, a.iters))
        tp.append(_window(plain, a.iters))
    row = {"criterion": what, "shape": shape, "native_us": round(statistics.mean(tn), 2), "native_spread_us": round(statistics.stdev(tn), 2),
           "torch_us": round(statistics.mean(tp), 2), "torch_spread_us": round(statistics.stdev(tp), 2),
           "speedup": round(statistics.mean(tp) / statistics.mean(tn), 2), "windows": a.windows, "iters": a.iters,
           "value_native": float(v_n), "value_torch": float(v_p.detach()), "grad_rel_diff": agree}
    print(json.dumps(row), flush=True)
    if not a.no_launch_count:           # after the timing line: the profiler is the one part of this tool that is not plain launches
        print(json.dumps({"criterion": what, "shape": shape, "native_launches": _launches(native), "torch_launches": _launches(plain)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8x1x256x256,1x1x1024x1024")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=12)
    ap.add_argument("--no-launch-count", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ssim_loss needs a GPU")
    _prewarm(0.8)
    for shape in a.shapes.split(","):
        B, C, H, W = (int(v) for v in shape.split("x"))
        p, t = make_pair(B * C, H, W, 17)
        pred, target = torch.from_numpy(p).cuda().view(B, C, H, W), torch.from_numpy(t).cuda().view(B, C, H, W)
        leaf = pred.clone().requires_grad_(True)
        ssim_crit, l2_crit = train_utils.SSIMMeanLoss(pred.device), train_utils.L2MeanLoss(pred.device)

        def plain_of(fn):
            def run():
                leaf.grad = None
                v = fn(leaf, target)
                v.backward()
                return v, leaf.grad
            return run

        _compare("ssim", [B, C, H, W], lambda: ssim_crit(pred, target), plain_of(ssim_loss_torch), a)
        _compare("l2", [B, C, H, W], lambda: l2_crit(pred, target), plain_of(F.mse_loss), a)


if __name__ == "__main__":
    main()
