"""Generates tests/golden/conv_pack_digests.json: SHA-256 digests of what sstem_conv3x3_pack_weights_f32 writes, per algorithm id
and layer shape.  A packed layout is a contract between a pack kernel and the MFMA kernel that reads it, and the digests pin every
layout bit for bit; regenerate them only where a layout is changed on purpose.  Needs the GPU.

Per id (ALGOS) and per (Cin, Cout) of SHAPES in both roles -- as listed and swapped -- the weights are
``torch.manual_seed(7); torch.randn(Cout, Cin, 3, 3) * 0.1`` made on the CPU.  Three calls: both destinations, the forward one alone,
the transposed one alone; buffers sized by sstem_conv3x3_packed_floats.  The file maps "<id>/<Cin>x<Cout>/<call>/<side>" to the digest
of the destination's int32 view.  For F16X3 only what is defined is hashed: float 0 (the bound) and [4 : n - 1024] -- floats 1 to 3 of
the header and the trailing amax word are scratch (test_conv_f16train_gpu.py compares the same range).

    python tests/golden/make_conv_pack_golden.py [out.json]
"""
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(REPO, "sstem-restoration_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)
import hipnn.functional as HF  # noqa: E402
import sstem_native  # noqa: E402

# (8, 24) .. (33, 3): the layers of test_group_weight_packing_after_the_optimiser_step (32 vs 64 output-channel blocks, ragged on both
# axes); 51 = 3 x 16 + 3 is the tap-row tail chunk under X6 and F16X3 and must not be one under X3; (130, 72): more than one 64-channel block
SHAPES = [(8, 24), (24, 40), (40, 33), (33, 3), (51, 35), (130, 72)]
ALGOS = {"mfma": HF.ALGO_MFMA, "bf16": HF.ALGO_MFMA_BF16, "bf16x3": HF.ALGO_MFMA_BF16X3, "bf16x6": HF.ALGO_MFMA_BF16X6,
         "f16x3": HF.ALGO_MFMA_F16X3}
CALLS = {"both": (True, True), "forward": (True, False), "transposed": (False, True)}
AMAX_WORD = 1024


def cases():
    return [c for s in SHAPES for c in (s, s[::-1])]


def _digest(buf, n, f16):
    v = buf[:n].view(torch.int32).cpu()
    if f16:
        v = torch.cat([v[:1], v[4:n - AMAX_WORD]])
    return hashlib.sha256(v.numpy().tobytes()).hexdigest()


def generate():
    lib = sstem_native.load_library()
    out = {}
    for name, algo in ALGOS.items():
        for Cin, Cout in cases():
            torch.manual_seed(7)
            w = (torch.randn(Cout, Cin, 3, 3) * 0.1).cuda()
            n_f = lib.sstem_conv3x3_packed_floats(Cin, Cout, algo)
            n_t = lib.sstem_conv3x3_packed_floats(Cout, Cin, algo)
            assert n_f > 0 and n_t > 0
            for call, (fwd, tr) in CALLS.items():
                ws_f = torch.zeros(n_f, device="cuda") if fwd else None
                ws_t = torch.zeros(n_t, device="cuda") if tr else None
                rc = lib.sstem_conv3x3_pack_weights_f32(w.data_ptr(), Cin, Cout, algo, ws_f.data_ptr() if fwd else None,
                                                        ws_t.data_ptr() if tr else None, None)
                assert rc == 0, (name, Cin, Cout, call, rc)
                torch.cuda.synchronize()
                key = "%s/%dx%d/%s/" % (name, Cin, Cout, call)
                if fwd:
                    out[key + "forward"] = _digest(ws_f, n_f, name == "f16x3")
                if tr:
                    out[key + "transposed"] = _digest(ws_t, n_t, name == "f16x3")
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "conv_pack_digests.json")
    data = generate()
    with open(path, "w") as f:
        json.dump(data, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", path, len(data), "digests,", os.path.getsize(path), "bytes")
