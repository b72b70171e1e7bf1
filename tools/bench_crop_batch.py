#!/usr/bin/env python
"""Developer benchmark: training batches cut from a device-resident set (data/resident.py: per batch one upload of the integer tables
and one launch of the oriented gather, include/sstem_batch.h) against the host formulation they replace -- the numpy restatement
tests/crop_ref.py (crop, orientation, replication, / 255) plus the upload of what that formulation uploads.

  interp   InterpBatcher.batch, B = 8 at 256 x 256              vs  crop_ref.interp_sample per sample + the 6 + 1 fp32 planes uploaded
  fusion   FoldSynthesizer.batch_resident, B = 16 / 32, 400 -> 256  vs  crop_ref.fusion_crops per sample + the two uint8 crops uploaded, then
           FoldSynthesizer.batch on them (the batch of tools/bench_fold.py, whose crops come from the host)

Both paths of a row draw from ``random.Random(seed)`` with the same seeds.  The first device batch of each row is checked bit for bit
against crop_ref (and, for the fusion row, tests/fold_ref.py for the folds it reports).  Each path is timed between two device events
and by the wall clock ended by a synchronise, ``--windows`` windows of ``--iters`` batches after a warm-up; ``gather_us`` is the
enqueue-to-finish time of the launch alone (tables already on the device).  The spread is the sample standard deviation of a path's
window means.  Prints one JSON line per row.  Run tools/bench_fold.py on the same box for the batch whose crops are uploaded from
pageable memory without the host crop.

    timeout 900 python tools/bench_crop_batch.py
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "sstem-restoration_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import crop_ref as C  # noqa: E402
import fold_ref as R  # noqa: E402
from data.fold_degradation import FoldSynthesizer  # noqa: E402
from data.interp_batch import IFNET_CHANNELS, InterpBatcher  # noqa: E402
from data.resident import AugFlags, ResidentImages, crop_f32, crop_u8, sample_table  # noqa: E402


def _prewarm(seconds):
    """An idle MI355X needs a few hundred ms under load to reach its clocks."""
    a = torch.randn(4096, 4096, device="cuda")
    t0 = time.time()
    while time.time() - t0 < seconds:
        (a @ a).sum().item()


def _bits_equal(t, want):
    got = t.cpu().numpy()
    return got.shape == want.shape and np.array_equal(got.view(np.uint32) if got.dtype == np.float32 else got, want.view(np.uint32) if want.dtype == np.float32 else want)


def timed(fn, seeds, windows):
    """fn(seed) per batch -> (wall mean, wall spread, event mean, event spread) in microseconds"""
    for s in seeds[:5]:
        fn(s)
    torch.cuda.synchronize()
    wall, ev = [], []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for s in seeds:
            fn(s)
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) / len(seeds) * 1e6)
        ev.append(e0.elapsed_time(e1) / len(seeds) * 1e3)
    sd = (lambda v: statistics.stdev(v) if len(v) > 1 else 0.0)
    return round(statistics.mean(wall), 1), round(sd(wall), 1), round(statistics.mean(ev), 1), round(sd(ev), 1)


def launch_alone(fn, windows, reps=200):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps * 1e3)
    return round(statistics.mean(out), 2), round(statistics.stdev(out), 2) if len(out) > 1 else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=24)
    ap.add_argument("--image-size", type=int, default=1024)
    ap.add_argument("--interp-batch", type=int, default=8)
    ap.add_argument("--interp-crop", type=int, default=256)
    ap.add_argument("--fusion-batches", default="16,32")
    ap.add_argument("--fusion-crop", type=int, default=400)
    ap.add_argument("--det-size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--host-iters", type=int, default=10)
    ap.add_argument("--host-windows", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_crop_batch needs a GPU")
    _prewarm(0.8)
    images = [C.image(3000 + i, a.image_size, a.image_size) for i in range(a.images)]
    t0 = time.perf_counter()
    resident = ResidentImages(images, "cuda:0")
    torch.cuda.synchronize()
    upload_once_us = (time.perf_counter() - t0) * 1e6
    seeds = [555 + i for i in range(a.iters)]
    common = {"resident_images": a.images, "resident_bytes": resident.nbytes, "resident_upload_once_us": round(upload_once_us, 0),
              "windows": a.windows, "iters": a.iters, "host_windows": a.host_windows, "host_iters": a.host_iters, "threads": torch.get_num_threads()}

    # ---- interp ---------------------------------------------------------------------------------------------------------------------
    B, S = a.interp_batch, a.interp_crop
    triplets = [(i, i + 1, i + 2) for i in range(a.images - 2)]
    shapes = [images[t[0]].shape for t in triplets]
    flags = AugFlags(*C.ALL_FLAGS)
    batcher = InterpBatcher(resident, triplets, S, flags)

    def host_interp(seed):
        rng = random.Random(seed)
        pairs = [C.interp_sample(images, triplets, C.draw_sample(rng, C.ALL_FLAGS, shapes, (S, S)), (S, S)) for _ in range(B)]
        im = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
        lb = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
        return im, lb

    im, lb = batcher.batch(random.Random(seeds[0]), B)
    him, hlb = host_interp(seeds[0])
    same = torch.equal(im.view(torch.int32), him.view(torch.int32)) and torch.equal(lb.view(torch.int32), hlb.view(torch.int32))
    dev = timed(lambda s: batcher.batch(random.Random(s), B, (im, lb)), seeds, a.windows)
    host = timed(host_interp, seeds[:a.host_iters], a.host_windows)
    table = sample_table(*batcher.draw(random.Random(seeds[0]), B), resident.device)
    gather = launch_alone(lambda: crop_f32(resident, table, S, S, IFNET_CHANNELS, 6, 0, im, lb), a.windows)
    row = {"what": "interp batch", "B": B, "crop": [S, S], "device_wall_us": dev[0], "device_wall_spread_us": dev[1], "device_event_us": dev[2],
           "device_event_spread_us": dev[3], "gather_us": gather[0], "gather_spread_us": gather[1], "host_wall_us": host[0],
           "host_wall_spread_us": host[1], "host_over_device_wall": round(host[0] / dev[0], 1), "upload_bytes_device": 4 * B * 6,
           "upload_bytes_host": 7 * 4 * B * S * S, "first_batch_bits_equal_crop_ref": bool(same)}
    row.update(common)
    print(json.dumps(row), flush=True)

    # ---- fusion ---------------------------------------------------------------------------------------------------------------------
    S, det = a.fusion_crop, a.det_size
    pairs = [(i, i + 1) for i in range(0, a.images - 1, 2)]
    shapes = [images[p[0]].shape for p in pairs]
    fflags = AugFlags(*C.FUSION_FLAGS)
    synth = FoldSynthesizer(det, 100)
    for B in (int(v) for v in a.fusion_batches.split(",")):
        def device_fusion(seed):
            return synth.batch_resident(resident, pairs, random.Random(seed), B, S, fflags)

        def host_fusion(seed):
            rng = random.Random(seed)
            crops = [C.fusion_crops(images, pairs, C.draw_sample(rng, C.FUSION_FLAGS, shapes, (S, S)), (S, S)) for _ in range(B)]
            clean, interp = np.stack([c[0] for c in crops]), np.stack([c[1] for c in crops])
            return synth.batch(torch.from_numpy(clean).cuda(), torch.from_numpy(interp).cuda(), rng), clean, interp

        got = device_fusion(seeds[0])
        _, clean, interp = host_fusion(seeds[0])
        same = True
        for i in range(B):
            ref = R.degrade(clean[i], interp[i], R.scalars(*got.folds[i]), synth.window(S))
            same = same and _bits_equal(got.im[i], ref["im"]) and _bits_equal(got.lb[i], ref["lb"])
        stats = {"rounds": 0, "n": 0}

        def counted(seed):
            b = device_fusion(seed)
            stats["rounds"] += b.rounds
            stats["n"] += 1

        dev = timed(counted, seeds, a.windows)
        host = timed(host_fusion, seeds[:a.host_iters], a.host_windows)
        rng = random.Random(seeds[0])
        rows = [C.draw_sample(rng, C.FUSION_FLAGS, shapes, (S, S)) for _ in range(B)]
        table = sample_table([(d[1], d[2], C.orientation_code(*d[3])) for d in rows], [pairs[d[0]] for d in rows], resident.device)
        buf = crop_u8(resident, table, S, S)
        gather = launch_alone(lambda: crop_u8(resident, table, S, S, buf), a.windows)
        row = {"what": "fusion batch", "B": B, "crop": [S, S], "window": [det, det], "device_wall_us": dev[0], "device_wall_spread_us": dev[1],
               "device_event_us": dev[2], "device_event_spread_us": dev[3], "rounds_per_batch": round(stats["rounds"] / stats["n"], 2),
               "gather_us": gather[0], "gather_spread_us": gather[1], "host_wall_us": host[0], "host_wall_spread_us": host[1],
               "host_over_device_wall": round(host[0] / dev[0], 1), "upload_bytes_device": 4 * B * 5, "upload_bytes_host": 2 * B * S * S,
               "first_batch_bits_equal_refs": bool(same)}
        row.update(common)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
