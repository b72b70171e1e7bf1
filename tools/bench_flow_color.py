#!/usr/bin/env python
"""Developer benchmark: the flow colour code and the SFF image tail on the device (include/sstem_display.h) against the host path they
replace, at the inference scripts' size.

  colour entry   sstem_flow_color_u8 on [B,2,1024,1024] fp32, B = 1 / 8: both launches, the workspace resident
  tail entry     sstem_sff_outputs_u8 on pred [B,1024,1024], warped [B,3,1024,1024], interp [B,1024,1024] uint8: all three outputs
  host colour    the flow downloaded (pageable memory, as the scripts do), then per image the numpy restatement
                 tests/flow_color_ref.flow_to_image on one core -- the reference's own arithmetic
  host tail      pred and warped downloaded, then tests/flow_color_ref.sff_outputs
  stream bound   the time a pure stream of the same bytes would take at the measured HBM copy rate (6.29 TB/s, MI355X float4 copy):
                 colour 8 B read twice and 3 B written per pixel, tail 16 B + 1 B read and 5 B written per pixel

The device rows are checked against the restatement first (the colour inside its range over the angle steps, the tail bit for bit).
Each entry is timed between two device events over ``--reps`` back-to-back calls, ``--windows`` windows; the host path by the wall
clock.  Prints one JSON line per row.

    timeout 600 python tools/bench_flow_color.py
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "sstem-restoration_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import flow_color_ref as R  # noqa: E402
import sstem_native  # noqa: E402
from bench_crop_batch import _prewarm, launch_alone  # noqa: E402

HBM_COPY_BYTES_PER_S = 6.29e12          # measured float4 copy on MI355X
COLOUR_BYTES_PER_PIXEL = 8 + 8 + 3      # the flow read by both launches, three bytes written
TAIL_BYTES_PER_PIXEL = 4 + 12 + 1 + 5   # pred, warped, interp read; pred_u8, warped_rgb, stitch written


def host_timed(fn, windows):
    if windows < 1:                     # --host-windows 0: a profiling run of the entries alone
        return None, None
    out = []
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return round(statistics.mean(out), 1), round(statistics.stdev(out), 1) if len(out) > 1 else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--host-windows", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_flow_color needs a GPU")
    _prewarm(0.8)
    lib = sstem_native.load_library()
    S = a.size
    stream = torch.cuda.current_stream().cuda_stream
    for B in (int(v) for v in a.batches.split(",")):
        rng = np.random.default_rng(100 + B)
        y, x = np.mgrid[0:S, 0:S].astype(np.float32)
        smooth = np.stack([4 * np.sin(x / 90) + 0.004 * (y - S / 2), 3 * np.cos(y / 70) - 0.003 * (x - S / 3)])
        flow_np = (smooth[None] * (1 + np.arange(B, dtype=np.float32))[:, None, None, None]
                   + 0.2 * rng.standard_normal((B, 2, S, S), dtype=np.float32)).astype(np.float32)
        pred_np = rng.random((B, S, S), dtype=np.float32)
        warped_np = np.repeat(rng.random((B, 1, S, S), dtype=np.float32), 3, 1) * (rng.random((B, 1, S, S), dtype=np.float32) > 0.02)
        interp_np = rng.integers(0, 256, size=(B, S, S), dtype=np.uint8)
        flow, pred, warped, interp = (torch.from_numpy(v).cuda() for v in (flow_np, pred_np, warped_np, interp_np))
        ws = torch.empty(max(64, int(lib.sstem_flow_color_workspace_bytes(B))), dtype=torch.uint8, device="cuda")
        rgb = torch.empty((B, S, S, 3), dtype=torch.uint8, device="cuda")
        pred_u8, stitch = torch.empty((B, S, S), dtype=torch.uint8, device="cuda"), torch.empty((B, S, S), dtype=torch.uint8, device="cuda")
        warped_rgb = torch.empty((B, S, S, 3), dtype=torch.uint8, device="cuda")

        def colour():
            sstem_native.check(lib.sstem_flow_color_u8(flow.data_ptr(), B, S, S, 0, rgb.data_ptr(), ws.data_ptr(), stream), "sstem_flow_color_u8")

        def tail():
            sstem_native.check(lib.sstem_sff_outputs_u8(pred.data_ptr(), warped.data_ptr(), interp.data_ptr(), B, S, S, pred_u8.data_ptr(),
                                                        warped_rgb.data_ptr(), stitch.data_ptr(), stream), "sstem_sff_outputs_u8")

        def host_colour():
            hwc = flow.permute(0, 2, 3, 1).cpu().numpy()
            return [R.flow_to_image(im) for im in hwc]

        def host_tail():
            return R.sff_outputs(pred.cpu().numpy(), warped.cpu().numpy(), interp_np)

        # the device rows against the restatement, image 0
        colour()
        tail()
        torch.cuda.synchronize()
        lo, hi, step0 = R.byte_range(np.ascontiguousarray(flow_np[0].transpose(1, 2, 0)))
        got = rgb[0].cpu().numpy()
        inside = bool(((got >= lo) & (got <= hi)).all())
        ref_tail = R.sff_outputs(pred_np, warped_np, interp_np)
        tail_same = all(np.array_equal(t.cpu().numpy(), r) for t, r in zip((pred_u8, warped_rgb, stitch), ref_tail))
        if not inside or not tail_same:
            raise SystemExit("B = %d: the device bytes do not match the restatement (colour inside range: %s, tail equal: %s)" % (B, inside, tail_same))

        pixels = B * S * S
        c = launch_alone(colour, a.windows, a.reps)
        t = launch_alone(tail, a.windows, a.reps)
        hc = host_timed(host_colour, a.host_windows)
        ht = host_timed(host_tail, a.host_windows)
        row = {"what": "flow colour code and SFF image tail", "shape": [B, 2, S, S], "reps": a.reps, "windows": a.windows,
               "colour_entry_us": c[0], "colour_entry_spread_us": c[1],
               "colour_stream_bound_us": round(pixels * COLOUR_BYTES_PER_PIXEL / HBM_COPY_BYTES_PER_S * 1e6, 2),
               "tail_entry_us": t[0], "tail_entry_spread_us": t[1],
               "tail_stream_bound_us": round(pixels * TAIL_BYTES_PER_PIXEL / HBM_COPY_BYTES_PER_S * 1e6, 2),
               "host_colour_us": hc[0], "host_colour_spread_us": hc[1], "host_tail_us": ht[0], "host_tail_spread_us": ht[1],
               "host_windows": a.host_windows, "colour_bytes_differing_from_step0_image0": int((got != step0).sum()),
               "checked": "colour inside the restatement's range, tail bit for bit"}
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
