"""Generates tests/golden/conv_launch_trace.json: for every route of hipnn.functional's convolution layer, the native launches it
issues -- entry point, every integer and float argument, which pointer arguments are given, and the stream -- in order.  The file
pins WHICH entry a call reaches with WHAT arguments; tests/test_conv_launch_trace_gpu.py compares today's trace with it case by
case.  Regenerate it only where a route is changed on purpose; a refactor of the Python layer does not.  Needs the GPU.

``generate()`` puts a recording proxy in place of the object ``sstem_native.load_library()`` returns (and takes it out again).  The
proxy forwards every call.  Pure size / support queries (QUERIES: functions of their integer arguments that launch nothing;
hipnn answers them from a dictionary after the first call) are not logged.  Of every other call it logs ``[name, arg, ...]``: integers
and floats as they are, a ``c_void_p`` argument (by the prototype's argtypes in sstem_native.C_ABI) as "ptr" or "null", and the
stream argument as "calling" or "side" (hipnn's weight-gradient side stream).

    python tests/golden/make_conv_launch_trace.py [out.json]
"""
import ctypes
import json
import os
import sys

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(REPO, "sstem-restoration_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)
import dataparallel as dp  # noqa: E402
import hipnn.functional as HF  # noqa: E402
import sstem_native  # noqa: E402
from hipnn.fused import FusedSequential  # noqa: E402

QUERY_SUFFIXES = ("_floats", "_floats_algo", "_supported", "_bytes", "_bytes_bf16coef", "_partials", "_count")
QUERIES = {n for n in sstem_native.C_ABI if n.endswith(QUERY_SUFFIXES)} | {"sstem_version", "sstem_status_string", "sstem_last_error"}
# the stream is the last pointer of every prototype that takes one, except:
STREAM_INDEX = {"sstem_conv3x3_forward_scaled_strided_f32": 20,       # (the pooled output comes behind it)
                "sstem_conv3x3_pack_group_entry": None}               # (a host call: fills one row of the group table)


def _stream_index(name, argtypes):
    if name in STREAM_INDEX:
        return STREAM_INDEX[name]
    ptrs = [i for i, t in enumerate(argtypes) if t is ctypes.c_void_p]
    return ptrs[-1] if ptrs else None


class _Recorder(object):
    """Stands in for the loaded library: every attribute is the real function behind a logging wrapper."""

    def __init__(self, real):
        self.__dict__["real"] = real
        self.__dict__["log"] = []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name in QUERIES or name not in sstem_native.C_ABI:
            return fn
        argtypes = sstem_native.C_ABI[name][1]
        si = _stream_index(name, argtypes)
        log = self.log

        def call(*args):
            assert len(args) == len(argtypes), name
            row = [name]
            for i, (a, t) in enumerate(zip(args, argtypes)):
                if i == si:
                    side = {s.cuda_stream for s in HF._side_streams.values()}
                    row.append("side" if a in side else "calling")
                elif t is ctypes.c_void_p:
                    row.append("null" if a is None else "ptr")
                elif t is ctypes.c_float:
                    row.append(float(a))
                else:
                    row.append(int(a))
            log.append(row)
            return fn(*args)
        self.__dict__[name] = call           # (built once per entry point)
        return call


class _knobs(object):
    """``with _knobs(_MASK_FUSION=False): ...`` -- module globals of hipnn.functional for the length of a case."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.prev = {k: getattr(HF, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(HF, k, v)

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            setattr(HF, k, v)
        return False


def _tensors(shape, k=3, seed=3):
    N, Cin, H, W, Cout = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g).cuda()
    w = (torch.randn(Cout, Cin, k, k, generator=g) * 0.1).cuda()
    b = torch.randn(Cout, generator=g).cuda()
    return x, w, b


def _recorded(shape, act=HF.ACT_RELU, k=3, **kw):
    """conv2d_fused forward + backward with gradients for input, weight and bias."""
    x, w, b = _tensors(shape, k)
    x.requires_grad_(); w.requires_grad_(); b.requires_grad_()
    out = HF.conv2d_fused(x, w, b, None, None, act, 0.0, **kw)
    out.backward(torch.ones_like(out))


def _case_bn_part():
    x, w, b = _tensors((1, 8, 5, 7, 3))
    conv = nn.Conv2d(8, 3, 3, padding=1).cuda()
    x.requires_grad_()
    part = HF.bn_partials_for(x, conv)
    assert part is not None
    out = HF.conv2d_fused(x, conv.weight, conv.bias, owner=conv, bn_part=part)
    out.backward(torch.ones_like(out))


def _inference(kind):
    """Nothing recorded, owner= a module, the forced fp16 id (shapes of test_conv_f16x3_gpu.py); every call twice."""
    N, Cin, H, W, Cout = shape = (1, 6, 48, 96, 32)
    x, w, b = _tensors(shape)
    conv = nn.Conv2d(Cin, Cout, 3, padding=1).cuda().requires_grad_(False)
    pool = nn.MaxPool2d(2)
    with torch.no_grad():
        conv.weight.copy_(w); conv.bias.copy_(b)
        for _ in range(2):
            if kind == "plain":
                HF.conv2d_fused(x, conv.weight, conv.bias, None, None, HF.ACT_RELU, 0.0, owner=conv)
            elif kind == "residual":
                res = torch.ones(N, Cout, H, W, device="cuda")
                HF.conv2d_fused(x, conv.weight, conv.bias, None, None, HF.ACT_LEAKY, 0.2, owner=conv, residual=res, res_scale=0.5)
            elif kind == "channel_block":
                big = torch.zeros(N, Cout + 5, H, W, device="cuda")
                assert HF.strided_store_ok(x, conv, big[:, 5:])
                HF.conv2d_fused(x, conv.weight, conv.bias, None, None, HF.ACT_RELU, 0.0, owner=conv, out=big[:, 5:])
            elif kind == "blocked":
                assert HF.blocked_store_ok(x, conv)
                HF.conv2d_fused(x, conv.weight, conv.bias, None, None, HF.ACT_RELU, 0.0, owner=conv, out_blocked=True)
            else:
                granted = HF.pooled_store_ok(x, conv, pool)
                assert granted == HF.POOL_MAX
                pooled = x.new_empty((N, Cout, H // 2, W // 2))
                HF.conv2d_fused(x, conv.weight, conv.bias, None, None, HF.ACT_RELU, 0.0, owner=conv, pool_out=pooled, pool_kind=granted,
                                pool_only=(kind == "pool_only"))


def _case_stream_small():
    shape = (1, 32, 1024, 1024, 2)
    assert HF._stream_small_ok(*shape)
    x, w, b = _tensors(shape)
    owner = nn.Module()
    with torch.no_grad():
        for _ in range(2):
            HF.conv2d_fused(x, w, b, None, None, HF.ACT_NONE, 0.0, owner=owner)
    assert not owner.__dict__.get("_sstem_packs")


def _convT(shape, recorded, calls=1):
    N, Cin, H, W, C = shape
    torch.manual_seed(11)
    x = torch.randn(N, Cin, H, W, device="cuda")
    m = nn.ConvTranspose2d(Cin, C, 3, stride=2, padding=1, output_padding=1).cuda()
    if recorded:
        x.requires_grad_()
        out = HF.conv_transpose3x3s2_fused(x, m.weight, m.bias, None, None, HF.ACT_RELU, 0.0, owner=m)
        out.backward(torch.ones_like(out))
    else:
        m.requires_grad_(False)
        with torch.no_grad():
            for _ in range(calls):
                HF.conv_transpose3x3s2_fused(x, m.weight, m.bias, None, None, HF.ACT_LEAKY, 0.2, owner=m)


def _case_convT_subpixel():
    torch.manual_seed(11)
    x = torch.randn(1, 16, 9, 20, device="cuda")
    m = nn.ConvTranspose2d(16, 32, 3, stride=2, padding=1, output_padding=1).cuda().requires_grad_(False)
    assert HF._convT_subpixel_ok(x, m.weight, m, False, None)
    big = torch.zeros(1, 32 + 3, 18, 40, device="cuda")
    with torch.no_grad():
        for _ in range(2):
            HF.conv_transpose3x3s2_fused(x, m.weight, m.bias, None, None, HF.ACT_LEAKY, 0.2, owner=m)
        HF.conv_transpose3x3s2_fused(x, m.weight, m.bias, None, None, HF.ACT_NONE, 0.0, owner=m, out=big[:, 3:])


def _case_chain():
    torch.manual_seed(5)
    convs = [nn.Conv2d(16, 24, 3, padding=1).cuda(), nn.Conv2d(24, 16, 3, padding=1).cuda()]
    x = torch.randn(1, 16, 32, 64, device="cuda", requires_grad=True)
    assert HF.conv_chain_ok(x, convs)
    out = HF.conv_chain(x, convs, [(HF.ACT_RELU, 0.0), (HF.ACT_RELU, 0.0)])
    out.backward(torch.ones_like(out))


def _sinks(with_convT):
    """One backward of a small FusedSequential whose parameters live in a FlatGradBucket."""
    torch.manual_seed(71)
    if with_convT:
        net = FusedSequential(nn.ConvTranspose2d(8, 4, 3, stride=2, padding=1, output_padding=1), nn.ReLU(), nn.Conv2d(4, 6, 3, padding=1)).cuda()
    else:
        net = FusedSequential(nn.Conv2d(8, 24, 3, padding=1), nn.ReLU(), nn.Conv2d(24, 16, 3, padding=1)).cuda()
    bucket = dp.FlatGradBucket(net.parameters())
    x = torch.randn(2, 8, 16, 32, device="cuda")
    bucket.zero()
    net(x).square().mean().backward()
    bucket.allreduce_mean()


def _cases():
    """name -> (forced algorithm id, knobs, function)."""
    A = HF
    c = {}
    c["conv/auto"] = (A.ALGO_AUTO, {}, lambda: _recorded((2, 6, 13, 37, 10)))
    c["conv/bf16x6/mask_fused"] = (A.ALGO_MFMA_BF16X6, {}, lambda: _recorded((2, 40, 24, 64, 70)))
    c["conv/bf16x6/mask_separate"] = (A.ALGO_MFMA_BF16X6, {"_MASK_FUSION": False}, lambda: _recorded((2, 40, 24, 64, 70)))
    c["conv/f16x3"] = (A.ALGO_MFMA_F16X3, {}, lambda: _recorded((2, 40, 32, 64, 70)))      # 4096 pixels: the fp16 weight gradient measures its bounds
    c["conv/direct"] = (A.ALGO_DIRECT, {}, lambda: _recorded((2, 6, 13, 37, 10)))
    c["conv/k1"] = (A.ALGO_AUTO, {}, lambda: _recorded((2, 5, 9, 11, 4), k=1))
    c["conv/k5"] = (A.ALGO_AUTO, {}, lambda: _recorded((2, 5, 9, 11, 4), k=5))
    c["conv/bn_part"] = (A.ALGO_AUTO, {"_BN_FUSED_STATS": True}, _case_bn_part)
    for kind in ("plain", "residual", "channel_block", "blocked", "pooled", "pool_only"):
        c["inference/" + kind] = (A.ALGO_MFMA_F16X3, {}, lambda kind=kind: _inference(kind))
    c["inference/stream_small"] = (A.ALGO_AUTO, {}, _case_stream_small)
    c["convT/native"] = (A.ALGO_AUTO, {}, lambda: _convT((1, 8, 5, 6, 4), True))
    c["convT/native_inference"] = (A.ALGO_AUTO, {}, lambda: _convT((1, 8, 5, 6, 4), False, calls=2))
    c["convT/direct"] = (A.ALGO_DIRECT, {}, lambda: _convT((1, 8, 5, 6, 4), True))
    c["convT/zero_insert"] = (A.ALGO_MFMA_BF16, {}, lambda: _convT((1, 8, 5, 6, 4), True))
    c["convT/subpixel"] = (A.ALGO_MFMA_F16X3, {}, _case_convT_subpixel)
    c["chain/mask_fused"] = (A.ALGO_MFMA_BF16, {}, _case_chain)
    c["chain/mask_separate"] = (A.ALGO_MFMA_BF16, {"_MASK_FUSION": False}, _case_chain)
    for name, t in (("conv", False), ("convT", True)):
        c["sinks/%s/default" % name] = (A.ALGO_AUTO, {}, lambda t=t: _sinks(t))
        c["sinks/%s/side_stream" % name] = (A.ALGO_AUTO, {"_SIDE_WGRAD_MIN_FLOP": 0.0}, lambda t=t: _sinks(t))
        c["sinks/%s/grouped" % name] = (A.ALGO_AUTO, {"_WGRAD_GROUP": True}, lambda t=t: _sinks(t))
    return c


# the entry points a case is there for: generate() refuses a trace that does not reach them (a golden that quietly covers less)
REACHES = {
    "conv/auto": ["sstem_conv2d_forward_ex_f32", "sstem_conv2d_backward_weight_bias_ex_f32"],
    "conv/bf16x6/mask_fused": ["sstem_conv3x3_forward_masked_f32", "sstem_conv3x3_backward_weight_masked_f32"],
    "conv/bf16x6/mask_separate": ["sstem_conv2d_forward_ex_f32", "sstem_conv2d_backward_weight_bias_ex_f32"],
    "conv/f16x3": ["sstem_conv3x3_forward_scaled_masked_f32", "sstem_conv3x3_backward_weight_scaled_masked_f32", "sstem_amax_f32"],
    "conv/bn_part": ["sstem_conv2d_forward_ex_f32"],
    "inference/plain": ["sstem_conv3x3_forward_scaled_strided_f32"],
    "inference/pool_only": ["sstem_conv3x3_forward_scaled_strided_f32"],
    "inference/stream_small": ["sstem_conv3x3_forward_scaled_strided_f32"],
    "convT/native": ["sstem_conv_transpose3x3s2_forward_ex_f32", "sstem_conv_transpose3x3s2_backward_ex_f32"],
    "convT/direct": ["sstem_conv_transpose3x3s2_forward_f32", "sstem_conv_transpose3x3s2_backward_f32"],
    "convT/zero_insert": ["sstem_conv2d_forward_ex_f32", "sstem_conv2d_backward_weight_bias_f32"],
    "convT/subpixel": ["sstem_conv3x3_forward_scaled_strided_f32"],
    "chain/mask_fused": ["sstem_conv3x3_forward_bf16io_masked", "sstem_conv3x3_backward_weight_bf16_masked"],
    "chain/mask_separate": ["sstem_conv3x3_forward_bf16io", "sstem_conv3x3_backward_weight_bf16in_ex"],
    "sinks/conv/grouped": ["sstem_wgrad_deferred_flush"],
    "sinks/convT/grouped": ["sstem_wgrad_deferred_flush"],
}


def _check_reach(name, rows):
    names = [r[0] for r in rows]
    for entry in REACHES.get(name, ()):
        assert entry in names, "%s no longer reaches %s: %s" % (name, entry, names)
    if name.startswith("sinks/"):
        acc = {"sstem_conv2d_backward_weight_bias_ex_f32": -3, "sstem_conv_transpose3x3s2_backward_ex_f32": -2}   # (before stream [, algo])
        flags = [r[1:][acc[r[0]]] for r in rows if r[0] in acc and r[1:][4 if r[0].startswith("sstem_conv_t") else 2] == "ptr"]
        streams = {r[1:][-2 if r[0].startswith("sstem_conv2d") else -1] for r in rows if r[0] in acc}
        assert flags and set(flags) == ({3} if name.endswith("grouped") else {1}), (name, flags)
        assert names.count("sstem_wgrad_deferred_flush") == (1 if name.endswith("grouped") else 0), (name, names)
        assert ("side" in streams) == name.endswith("side_stream"), (name, streams)


def generate():
    real = sstem_native.load_library()
    rec = _Recorder(real)
    out = {}
    sstem_native._lib = rec
    try:
        for name, (algo, knobs, fn) in _cases().items():
            del rec.log[:]
            with HF.algorithm(algo), _knobs(**knobs):
                fn()
            torch.cuda.synchronize()
            out[name] = [list(r) for r in rec.log]
            _check_reach(name, out[name])
    finally:
        sstem_native._lib = real
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "conv_launch_trace.json")
    data = generate()
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join("%s: [\n%s\n]" % (json.dumps(k), ",\n".join(" " + json.dumps(r) for r in v))
                                   for k, v in sorted(data.items())) + "\n}\n")
    print("wrote", path, len(data), "cases,", sum(len(v) for v in data.values()), "launches,", os.path.getsize(path), "bytes")
