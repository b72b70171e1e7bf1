#!/usr/bin/env python
"""Where a row pair of the blocked fused apply spends its time, from a -DSSTEM_PAIR_STAMP=1 build of the library:

    tools/build_ablate.sh stamp "-DSSTEM_PAIR_STAMP=1"
    SSTEM_NATIVE_LIB=build_ablate/libsstem_stamp.so SSTEM_GRAY_PAIR=2 python tools/pair_stamps.py            # sepconv_gray_mfma_pair
    SSTEM_NATIVE_LIB=build_ablate/libsstem_stamp.so SSTEM_GRAY_PAIR=3 python tools/pair_stamps.py 378,432,594  # ..._pair_hp, 4+4+6

Wave 0 of every workgroup writes s_memtime at five points of each pair: 0 pair start, 1 first MFMA (the waits for the B operand and
its skew are over), 2 and 3 two marks inside the pair, 4 pair end (stores issued).  The marks are the start of group 1 and of group 6
in the pair kernel, the start of pass 1 and of the last pass in the multi-pass kernel.  The argument is the number of MFMAs between
points 1-2, 2-3 and 3-4 (default: the pair kernel's 162,1080,162).  Reported over one C2 launch (B 8, 1024 x 1024):
    drain       = t1 - t0
    last_excess = (t4 - t3) - n34 / n23 * (t3 - t2)      the last stretch against the middle one at equal MFMA counts
both in clocks and as a share of the pair time t4 - t0.  The stamps themselves cost time: compare shares, not milliseconds.
"""
import ctypes, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "sstem-restoration_amd"))
import numpy as np
import torch
import sstem_native
from libs.sepconv.fused import coef_blocked_shape, interp_apply_gray_blocked

n12, n23, n34 = [int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "162,1080,162").split(",")]
B, H, W = 8, 1024, 1024
WGS, PER_WG = 2048, 80
raw = ctypes.CDLL(os.environ["SSTEM_NATIVE_LIB"])
raw.sstem_debug_pair_stamps.restype = ctypes.c_int
raw.sstem_debug_pair_stamps.argtypes = [ctypes.c_void_p, ctypes.c_longlong]
g = torch.Generator(device="cuda").manual_seed(1)
g1 = torch.rand(B, 1, H, W, device="cuda", generator=g)
g2 = torch.rand(B, 1, H, W, device="cuda", generator=g)
kb = [torch.rand(coef_blocked_shape(B, H, W), device="cuda", generator=g) / 25.5 for _ in range(4)]
for _ in range(300):                                   # clocks settled, steady state
    interp_apply_gray_blocked(g1, g2, *kb)
e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(50):
    interp_apply_gray_blocked(g1, g2, *kb)
e1.record(); torch.cuda.synchronize()
buf = np.zeros(WGS * PER_WG, dtype=np.uint64)
assert raw.sstem_debug_pair_stamps(buf.ctypes.data, buf.size) == 0, "no stamps: is SSTEM_NATIVE_LIB a -DSSTEM_PAIR_STAMP=1 build?"
t = buf.reshape(WGS, 2, 8, 5).astype(np.int64)
ok = (t != 0).all(axis=3)
assert ok.any(), "no pair was stamped: SSTEM_GRAY_PAIR must select a row-pair kernel (2 or 3)"
print("SSTEM_GRAY_PAIR=%s, %.1f us per launch with the stamps in; %d of %d pairs of wave 0 stamped; MFMAs between the marks %d / %d / %d"
      % (os.environ.get("SSTEM_GRAY_PAIR", "default"), e0.elapsed_time(e1) * 20, int(ok.sum()), ok.size, n12, n23, n34))
for ph in (0, 1, None):
    sel = ok if ph is None else ok & (np.arange(2)[None, :, None] == ph)
    d = t[sel]
    pair = d[:, 4] - d[:, 0]
    drain = d[:, 1] - d[:, 0]
    first, mid, last = d[:, 2] - d[:, 1], d[:, 3] - d[:, 2], d[:, 4] - d[:, 3]
    excess = last - mid * (float(n34) / n23)
    def line(name, v):
        print("   %-12s mean %9.0f  median %9.0f clocks   %5.1f %% of the pair time (mean / mean)" % (name, v.mean(), np.median(v), 100.0 * v.mean() / pair.mean()))
    print("phase %s: %d pairs, pair time mean %.0f median %.0f clocks" % ("0+1" if ph is None else ph, len(d), pair.mean(), np.median(pair)))
    line("drain", drain)
    line("t1..t2", first)
    line("t2..t3", mid)
    line("t3..t4", last)
    line("last_excess", excess)
    print("   clocks per MFMA: t1..t2 %.2f   t2..t3 %.2f   t3..t4 %.2f" % (first.mean() / n12, mid.mean() / n23, last.mean() / n34))
