#!/usr/bin/env python
"""Developer benchmark: the SFF training batch from the fold synthesis launches (data.fold_degradation.FoldSynthesizer.batch: upload
of two uint8 crops per sample, then per round one call of sstem_fold_degrade_u8 and one readback of the B counts) against the host
path it replaces -- the same degradation in numpy on full planes (tests/fold_ref.py: the flow on the whole S x S plane, the byte warp,
the mask, the centre crop, the rejection loop, the 6 + 1 fp32 planes) plus the host-to-device copy of the fp32 batch.

Both paths draw from ``random.Random(seed)`` with the same seeds; the host path redraws sample by sample and the device path round
by round, so beyond one sample they meet the same distribution of folds, not the same folds (``candidates_per_batch`` says how many
each drew).  The first device batch is checked bit for bit against tests/fold_ref.py for the folds it reports.
The device path is timed twice over the same calls: between two device events and by the wall clock ended by a synchronise (the
readback of every round stalls the host, which the events alone do not show); ``--windows`` windows of ``--iters`` batches after a
warm-up.  ``degrade_us`` is the enqueue-to-finish time of the launches alone (fold table already on the device, no readback) and
``readback_us`` the wall clock of one ``zero_count.cpu()`` on an idle stream: what a round pays for the host's decision.
The host path runs ``--host-iters`` batches per window by the wall clock, at the thread setting the process was started with.
The spread is the sample standard deviation of a path's window means.  Prints one JSON line per batch size.

    timeout 900 python tools/bench_fold.py
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

import fold_ref as R  # noqa: E402
from data.fold_degradation import FoldSynthesizer, degrade, draw_fold, fold_table  # noqa: E402


def _prewarm(seconds):
    """An idle MI355X needs a few hundred ms under load to reach its clocks."""
    a = torch.randn(4096, 4096, device="cuda")
    t0 = time.time()
    while time.time() - t0 < seconds:
        (a @ a).sum().item()


def host_batch(clean, interp, rng, det_size, min_zero):
    """The batch on the host, sample by sample as the reference's loader makes it, then uploaded.  Returns (im, lb, candidates)."""
    B, S, _ = clean.shape
    off = (S - det_size) // 2
    ims, lbs, drawn = [], [], 0
    f255 = np.float32(255)
    for i in range(B):
        while True:
            fold = draw_fold(rng, S, S)
            drawn += 1
            flow, _, mask = R.flow(R.scalars(*fold), S, S)
            deformed = (R.warp(clean[i], flow) * mask)[off:S - off, off:S - off]
            if int((deformed == 0).sum()) >= min_zero:
                break
        d = np.repeat(deformed[None], 3, 0)
        it = np.repeat(interp[i, off:S - off, off:S - off][None], 3, 0)
        ims.append(np.concatenate([d, it], 0).astype(np.float32) / f255)
        lbs.append(clean[i, off:S - off, off:S - off][None].astype(np.float32) / f255)
    im, lb = torch.from_numpy(np.stack(ims)).cuda(), torch.from_numpy(np.stack(lbs)).cuda()
    torch.cuda.synchronize()
    return im, lb, drawn


def device_batch(synth, clean, interp, rng):
    return synth.batch(torch.from_numpy(clean).cuda(), torch.from_numpy(interp).cuda(), rng)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="16,32")
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--det-size", type=int, default=256)
    ap.add_argument("--min-zero", type=int, default=100)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--host-iters", type=int, default=1)
    ap.add_argument("--host-windows", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fold needs a GPU")
    _prewarm(0.8)
    synth = FoldSynthesizer(a.det_size, a.min_zero)
    S = a.size
    for B in (int(v) for v in a.batches.split(",")):
        clean = np.stack([R.image(1000 + i, S, S) for i in range(B)])
        interp = np.stack([R.image(2000 + i, S, S) for i in range(B)])
        seeds = [555 + i for i in range(a.iters)]
        # one batch of either path; the device batch is checked against fold_ref for the folds it reports
        got = device_batch(synth, clean, interp, random.Random(seeds[0]))
        want_im, want_lb, want_drawn = host_batch(clean, interp, random.Random(seeds[0]), a.det_size, a.min_zero)
        assert tuple(want_im.shape) == tuple(got.im.shape) and tuple(want_lb.shape) == tuple(got.lb.shape)
        same = True
        for i in range(B):
            ref = R.degrade(clean[i], interp[i], R.scalars(*got.folds[i]), synth.window(S))
            same = same and np.array_equal(got.im[i].cpu().numpy().view(np.uint32), ref["im"].view(np.uint32)) \
                and np.array_equal(got.lb[i].cpu().numpy().view(np.uint32), ref["lb"].view(np.uint32))
        for s in seeds[:5]:
            device_batch(synth, clean, interp, random.Random(s))
        torch.cuda.synchronize()
        ev, wall, rounds, calls, drawn = [], [], 0, 0, 0
        for _ in range(a.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for s in seeds:
                b = device_batch(synth, clean, interp, random.Random(s))
                rounds, calls, drawn = rounds + b.rounds, calls + b.launches, drawn + b.drawn
            e1.record()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) / a.iters * 1e6)
            ev.append(e0.elapsed_time(e1) / a.iters * 1e3)
        # the launches alone, and one readback alone
        cl, it = torch.from_numpy(clean).cuda(), torch.from_numpy(interp).cuda()
        rng = random.Random(seeds[0])
        folds = fold_table([draw_fold(rng, S, S) for _ in range(B)], cl.device)
        out = degrade(cl, it, folds, synth.window(S))
        torch.cuda.synchronize()
        deg = []
        for _ in range(a.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                degrade(cl, it, folds, synth.window(S), out=out)
            e1.record()
            torch.cuda.synchronize()
            deg.append(e0.elapsed_time(e1) / 200 * 1e3)
        rb = []
        for _ in range(a.windows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(200):
                out.zero_count.cpu()
            rb.append((time.perf_counter() - t0) / 200 * 1e6)
        host = []
        for w in range(a.host_windows):
            t0 = time.perf_counter()
            for s in seeds[:a.host_iters]:
                host_batch(clean, interp, random.Random(s), a.det_size, a.min_zero)
            host.append((time.perf_counter() - t0) / a.host_iters * 1e6)
        n = a.windows * a.iters
        win = a.det_size * a.det_size
        row = {"what": "fold batch", "B": B, "plane": [S, S], "window": [a.det_size, a.det_size],
               "device_wall_us": round(statistics.mean(wall), 1), "device_wall_spread_us": round(statistics.stdev(wall), 1),
               "device_event_us": round(statistics.mean(ev), 1), "device_event_spread_us": round(statistics.stdev(ev), 1),
               "rounds_per_batch": round(rounds / n, 2), "entry_calls_per_batch": round(calls / n, 2), "kernels_per_entry_call": 2,
               "candidates_per_batch": round(drawn / n, 2),
               "degrade_us": round(statistics.mean(deg), 2), "degrade_spread_us": round(statistics.stdev(deg), 2),
               "degrade_store_bytes": B * win * (1 + 6 * 4 + 4) + 4 * B,
               "readback_us": round(statistics.mean(rb), 1), "readback_spread_us": round(statistics.stdev(rb), 1),
               "host_us": round(statistics.mean(host), 0), "host_spread_us": round(statistics.stdev(host), 0) if len(host) > 1 else None,
               "host_candidates_first_seed": want_drawn, "host_over_device_wall": round(statistics.mean(host) / statistics.mean(wall), 1),
               "upload_bytes_device": 2 * B * S * S, "upload_bytes_host": 7 * 4 * B * win, "threads": torch.get_num_threads(),
               "first_batch_bits_equal_fold_ref": bool(same),
               "windows": a.windows, "iters": a.iters, "host_windows": a.host_windows, "host_iters": a.host_iters}
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
