"""Generates tests/golden/capi_refusals.json: what libsstem_hip.so itself answers to calls it refuses, to empty-shape calls and to its
size / ``_supported`` queries -- the record tests/test_capi_refusals.py replays against later builds.  Nothing comes from the
reference; the library under csrc/ at the commit that is checked out is the source.  Run from the repo root, where NO device is
visible (pointers are small integers, not memory):

    HIP_VISIBLE_DEVICES=-1 python tests/golden/make_capi_refusals.py

File: {entry: {"args": [names], "base": [a call that passes validation], "answers": [[answer, [call, ...]], ...]}}, one answer and
the calls that got it per line.  For an entry that takes tensors a call is {name: value, ...}: the base with those arguments
replaced, "pointers" standing for every pointer argument; for the rest (no "base") it is the argument list.  Pointers are integers
or null; answer = [status, sstem_last_error() text]
(text null when the status is 0), or [value] for a query, or [value, [16 words]] where the call wrote its host out-parameter.
Two conditions hold for every row and are asserted here: a row with status 0 has every pointer null, and no row has status 4 or 5
(a call that passed validation and reached HIP is not a refusal and is dropped)."""
import ctypes
import glob
import itertools
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import capi_replay  # noqa: E402
from capi_replay import HOST16, REPO, call, sstem_native  # noqa: E402

_p, _i64, _int, _f = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float


def prototypes():
    """name -> argument names, from include/*.h"""
    out = {}
    for h in glob.glob(os.path.join(REPO, "include", "*.h")):
        text = re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        for name, args in re.findall(r"\b(sstem_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
            args = args.strip()
            out[name] = [] if args in ("", "void") else [re.findall(r"[A-Za-z_0-9]+", a)[-1] for a in args.split(",")]
    return out


INT_BASE = {"B": 2, "N": 2, "C": 3, "Cin": 16, "Cout": 16, "H": 8, "W": 8, "HW": 64, "planes": 4, "n": 64, "npix": 64, "replicas": 3,
            "workspace_floats": 1 << 40, "n_entries": 1, "total_blocks": 1, "bound_blocks": 1, "n_partials": 0, "step": 1,
            "output_image_stride": 0, "KH": 3, "KW": 3, "pad_h": 1, "pad_w": 1, "taps": 5, "is_max": 1, "frame_planes": 1}
FLOAT_BASE = {"slope": 0.25, "residual_scale": 1.0, "momentum": 0.5, "eps": 0.5, "lr": 0.5, "beta1": 0.5, "beta2": 0.5,
              "weight_decay": 0.0}
# what a call that passes validation looks like, where the defaults above do not give one
BASE = {
    "sstem_conv3x3_pack_weights_f32": {"algo": 2}, "sstem_conv3x3_pack_weights_group_f32": {"algo": 2},
    "sstem_conv3x3_pack_group_entry": {"algo": 2, "entry16": HOST16},
    "sstem_conv2d_forward_f32": {"algo": 2}, "sstem_conv2d_forward_ex_f32": {"algo": 2, "bn_partials": None},
    "sstem_conv3x3_forward_masked_f32": {"algo": 5}, "sstem_conv3x3_backward_weight_masked_f32": {"algo": 5},
    "sstem_conv3x3_forward_scaled_f32": {"algo": 6},
    "sstem_conv3x3_forward_scaled_strided_f32": {"algo": 6, "pooled_output": None},
    "sstem_conv3x3_first_layer_u8": {"Cout": 6},
    "sstem_conv_transpose3x3s2_forward_ex_f32": {"bn_partials": None},
    "sstem_conv2d_backward_weight_f32": {"algo": 2}, "sstem_conv2d_backward_weight_bias_f32": {"algo": 2},
    "sstem_conv2d_backward_weight_bias_ex_f32": {"algo": 2},
    "sstem_batchnorm_train_forward_ex_f32": {"partials": None}, "sstem_batchnorm_train_forward_amax_f32": {"partials": None},
}

# entries that hand their arguments to another entry unchanged (in this file's parent and now): the full probe lists go to that one
WRAPPERS = {"sstem_sepconv_forward_f32", "sstem_sepconv_backward_f32", "sstem_conv2d_forward_f32", "sstem_conv3x3_forward_scaled_f32",
            "sstem_conv2d_backward_weight_f32", "sstem_conv2d_backward_weight_bias_f32", "sstem_conv3x3_backward_weight_bf16in",
            "sstem_batchnorm_train_forward_f32", "sstem_batchnorm_train_forward_ex_f32", "sstem_batchnorm_train_backward_f32",
            "sstem_batchnorm_train_backward_ex_f32", "sstem_sepconv_backward_input_f32"}
BIG = [1 << 30, (1 << 30) + 1, 1 << 40, (1 << 40) + 1]
CH = [1 << 20, (1 << 20) + 1] + BIG
HW = [1 << 14, (1 << 14) + 2, 1 << 15, (1 << 15) + 2, (1 << 20) + 4] + BIG
PROBES = {     # single-argument values, by argument name
    "B": [-1, 0, 65535, 65536] + BIG, "N": [-1, 0, 65535, 65536] + BIG, "C": [-1, 0, 1, 4, 52] + BIG,
    "Cin": [-1, 0, 6, 8] + CH, "Cout": [-1, 0, 6, 128] + CH, "H": [-1, 0, 1, 4, 4588, 4589] + HW, "W": [-1, 0, 1, 6, 7, 32, 4588, 4589] + HW,
    "HW": [-1, 0, 1 << 31, (1 << 31) + 1], "planes": [-1, 0, (1 << 31) - 1, 1 << 31] + BIG, "n": [-1, 0, 1 << 40, (1 << 40) + 1], "npix": [-1, 0, 1 << 40, (1 << 40) + 1],
    "replicas": [-1, 0, 1024, 1025], "workspace_floats": [-1, 0, 1], "n_entries": [-1, 0, 1 << 20, (1 << 20) + 1], "total_blocks": [-1, 0],
    "bound_blocks": [-1, 0], "n_partials": [-1, 1], "step": [0, 2], "output_image_stride": [-1, 1, 16 * 8 * 8 - 1, 16 * 8 * 8, 16 * 8 * 8 + 4],
    "KH": [0, 1, 5, 6], "KW": [0, 1, 5, 6], "pad_h": [-1, 0, 2], "pad_w": [-1, 0, 2], "taps": [0, 1, 51, 1024, 1025],
    "act": [-1, 1, 2, 3], "weight_flags": [-1, 1, 2, 3, 4], "weight_transposed": [-1, 1, 2, 3, 4], "algo": [-1, 0, 1, 2, 3, 4, 5, 6, 7],
    "accumulate": [1, 3], "is_max": [0], "input_bf16": [1], "output_bf16": [1], "output_layout": [-1, 1, 2, 3], "pool_kind": [1, 2, 3],
    "blocked_coefficients": [1], "clamp01": [1],
}
SHAPES = [     # several arguments at once: either side of the products the file limits
    {"Cin": 46341, "Cout": 46341}, {"Cin": 46340, "Cout": 46341},                                   # Cin*Cout against 2^31
    {"H": 1 << 16, "W": 1 << 15}, {"H": 1 << 16, "W": (1 << 15) - 4},                                # H*W against 2^31
    {"N": 1 << 16, "Cin": 1 << 10, "H": 1 << 10, "W": 1 << 10}, {"N": (1 << 16) - 1, "Cin": 1 << 10, "H": 1 << 10, "W": 1 << 10},     # 2^46
    {"B": 1 << 16, "C": 1 << 10, "H": 974, "W": 974}, {"B": (1 << 16) - 1, "C": 1 << 10, "H": 974, "W": 974},
    {"H": 1 << 14, "W": 1 << 13}, {"H": (1 << 14) - 1, "W": 1 << 13}, {"H": 1 << 13, "W": 1 << 12}, {"H": (1 << 13) - 1, "W": 1 << 12},  # 8*H*W*4, 32*H*W*4 against 2^32
    {"output_layout": 2, "Cout": 128, "H": 8192, "W": 1024}, {"output_layout": 2, "Cout": 128, "H": 8191, "W": 1024},              # Cout*H*W*4 against 2^32
    {"output_layout": 2, "Cout": 64}, {"output_layout": 2, "Cout": 128, "Cin": 8}, {"output_layout": 2, "Cout": 128, "W": 6},
    {"output_layout": 2, "Cout": 128, "algo": 5}, {"output_layout": 2, "Cout": 128},
    {"output_layout": 1, "H": 1 << 14, "W": 4096}, {"output_layout": 1, "H": (1 << 14) - 1, "W": 4096}, {"output_layout": 1, "residual": None},
    {"output_layout": 1, "output_image_stride": 1 << 20}, {"output_layout": 1},
    {"pooled_output": 0x3000, "pool_kind": 1, "residual": None, "W": 32}, {"pooled_output": 0x3000, "pool_kind": 1, "residual": None, "W": 32, "H": 4},
    {"pooled_output": 0x3000, "pool_kind": 1, "residual": None, "W": 8}, {"pooled_output": 0x3000, "pool_kind": 1, "W": 32},
    {"pooled_output": 0x3000, "pool_kind": 3}, {"pooled_output": 0x3000, "pool_kind": 0}, {"pooled_output": 0x3000, "pool_kind": 2, "residual": None, "W": 32, "algo": 5},
    {"pooled_output": 0x3000, "pool_kind": 1, "residual": None, "W": 32, "output": None},
    {"algo": 1, "residual": None}, {"algo": 1, "residual": None, "weight_flags": 1}, {"algo": 1, "residual": None, "output_image_stride": 16 * 8 * 8},
    {"algo": 1, "residual": None, "output_image_stride": 16 * 8 * 8 + 4}, {"algo": 1, "residual": None, "Cout": 2, "Cin": 6},
    {"algo": 1, "residual": None, "N": 0}, {"algo": 1, "residual": None, "input": None}, {"algo": 1}, {"algo": 6, "input_amax": None}, {"algo": 5, "input_amax": None},
    {"KH": 5, "KW": 5, "pad_h": 2, "pad_w": 2}, {"KH": 5, "KW": 5, "pad_h": 2, "pad_w": 2, "algo": 1}, {"KH": 5, "KW": 5, "pad_h": 2, "pad_w": 2, "algo": 0},
    {"KH": 5, "KW": 5, "pad_h": 2, "pad_w": 2, "weight_transposed": 1}, {"KH": 1, "KW": 1, "pad_h": 0, "pad_w": 0, "algo": 3}, {"KH": 1, "KW": 1, "pad_h": 0, "pad_w": 0, "algo": 5},
    {"KH": 1, "KW": 1, "pad_h": 0, "pad_w": 0, "algo": 1, "grad_bias": None}, {"algo": 1, "weight_transposed": 1}, {"algo": 1, "grad_bias": None},
    {"bn_partials": 0x3000}, {"bn_partials": 0x3000, "scale": None, "shift": None, "residual": None}, {"bn_partials": 0x3000, "scale": None, "shift": None, "residual": None, "act": 1},
    {"bn_partials": 0x3000, "scale": None, "shift": None, "residual": None, "workspace_floats": 16 * 16 * 9 * 4},
    {"bn_partials": 0x3000, "scale": None, "shift": None, "residual": None, "algo": 5}, {"bn_partials": 0x3000, "scale": None, "shift": None, "residual": None, "algo": 3},
    {"bn_partials": 0x3000, "scale": None, "shift": None, "residual": None, "N": 1, "Cin": 512, "Cout": 512, "H": 2, "W": 2},
    {"residual": None, "algo": 3}, {"residual": None, "algo": 3, "W": 4097, "H": 4097, "Cin": 64, "Cout": 64}, {"algo": 5, "W": 4097, "H": 4097, "Cin": 64, "Cout": 64},
    {"W": 4097, "H": 4097, "Cin": 64, "Cout": 64, "N": 1}, {"W": 8192, "H": 8192, "Cin": 64, "Cout": 64, "N": 1}, {"W": 8192, "H": 8192, "Cin": 64, "Cout": 64, "N": 1, "output_bf16": 1},
    {"input_bf16": 1, "input_mask": None}, {"input_mask": None, "output_mask": None, "input": 0x1004}, {"input_mask": None, "output_mask": None, "W": 6},
    {"Cin": 0, "input": None}, {"N": 0, "accumulate": 1}, {"N": 0, "grad_weight": None}, {"N": 0, "grad_weight": None, "grad_bias": None, "Cin": 0},
    {"grad_input": None}, {"grad_input": None, "grad_weight": None}, {"grad_weight": None, "grad_bias": None}, {"grad_input": None, "input": None},
    {"grad_input": None, "workspace_floats": 0}, {"grad_weight": None, "grad_bias": None, "workspace_floats": 0}, {"grad_weight": None, "grad_bias": None, "weight": None},
    {"H": 1, "W": 1}, {"H": 1, "W": 1, "grad_output": None, "argmax": None}, {"H": 8, "W": 8, "argmax": None, "is_max": 0}, {"is_max": 0, "argmax": None},
    {"partials": 0x3000, "n_partials": 0}, {"partials": 0x3000, "n_partials": 1, "workspace": None}, {"C": 0, "grad_output": None, "input": None},
    {"C": 0}, {"C": 4, "B": 0}, {"C": 4, "H": 0}, {"H": 0, "grad_output": None, "vertical": None, "horizontal": None}, {"H": 0, "W": 0, "taps": 1}, {"taps": 51, "algo": 2},
    {"B": 65536, "H": 64, "W": 64}, {"B": 1, "H": 4588, "W": 4588}, {"B": 1, "H": 4589, "W": 4589}, {"B": 1, "H": 2896, "W": 2896}, {"B": 1, "H": 2897, "W": 2897},
    {"blocked_coefficients": 1, "B": 1, "H": 4589, "W": 4589}, {"blocked_coefficients": 1, "B": 1, "H": 4588, "W": 4588},
    {"algo": 2, "B": 1, "C": 1, "H": 4589, "W": 4589}, {"algo": 2, "B": 1, "C": 1, "H": 4588, "W": 4588},
    {"algo": 5, "workspace_floats": 0}, {"algo": 3, "workspace_floats": 0, "residual": None}, {"algo": 3, "workspace_floats": 0},
    {"bn_partials": 0x3000, "scale": None, "shift": None, "residual": None, "N": 1, "Cin": 512, "Cout": 512, "H": 16, "W": 16, "workspace_floats": 2359296},
    {"algo": 7, "residual": None}, {"algo": -1, "residual": None},
    {"packed_forward": None, "packed_transposed": None, "weight": None}, {"packed_forward": None}, {"table": None, "n_entries": 0},
]


def base_args(name, names, argtypes):
    out, k = [], 0
    for arg, t in zip(names, argtypes):
        if arg in BASE.get(name, {}):
            out.append(BASE[name][arg])
        elif t is _p:
            k += 1
            out.append(None if arg == "stream" else 0x1000 * k)     # 16-byte aligned, one value per tensor
        elif t is _f:
            out.append(FLOAT_BASE.get(arg, 0.5))
        else:
            out.append(INT_BASE.get(arg, 0))
    return out


def mutations(names, argtypes, base):
    """dicts {argument: value}: every pointer null / off 16-byte alignment, every probe value, every SHAPES entry that applies."""
    muts = []
    ptrs = [a for a, t, b in zip(names, argtypes, base) if t is _p and a != "stream" and b != HOST16]
    for a in ptrs:
        muts += [{a: None}, {a: 0x1004}]
    if len(ptrs) > 1:
        muts.append({a: None for a in ptrs})
    for a, t in zip(names, argtypes):
        if t is not _p:
            muts += [{a: v} for v in PROBES.get(a, [])]
    muts += [m for m in SHAPES if all(a in names for a in m)]
    return muts, ptrs


def apply(names, base, mut):
    return [mut.get(a, b) for a, b in zip(names, base)]


QUERY_SHAPES5 = [(8, 64, 512, 512, 64), (2, 512, 16, 16, 512), (1, 6, 9, 9, 51), (8, 6, 512, 512, 32), (8, 51, 512, 512, 51), (1, 512, 16, 16, 512),
                 (8, 64, 128, 128, 64), (16, 64, 256, 256, 64), (8, 6, 256, 256, 32), (1, 3, 1, 1, 2), (0, 64, 8, 8, 64), (1, -1, 8, 8, 64),
                 (8, 51, 1024, 1024, 51), (1, 64, 8192, 8192, 64), (1, 64, 8000, 8000, 64), (1, 4, 8192, 8192, 4), (1, 64, 4097, 4097, 64),
                 (1, 8, 4097, 4097, 8), (1, 64, 8, 8, 64), (1, 1, 1 << 16, 1 << 15, 1), (1, 1, 1 << 16, (1 << 15) - 1, 1), (1 << 16, 1 << 10, 1 << 10, 1 << 10, 1),
                 ((1 << 16) - 1, 1 << 10, 1 << 10, 1 << 10, 1), ((1 << 30) + 1, 1, 1, 1, 1), (1 << 30, 1, 1, 1, 1), (1, 1, 1, 1, (1 << 30) + 1), (2048, 16, 8, 8, 1024),
                 (2047, 16, 8, 8, 1024), (65536, 3, 8, 8, 32), (65535, 3, 8, 8, 32), (2, 16, 8, 8, 0), (2, 0, 8, 8, 16), (2, 16, 0, 8, 16), (2, 16, 8, 0, 16),
                 (2, 6, 8, 8, 6), (2, 6, 8, 6, 6), (2, 3, 64, 64, 2), (2, 16, 64, 64, 5), (1, 16, 1 << 14, 1 << 13, 16), (1, 16, (1 << 14) - 1, 1 << 13, 16)]
QUERY_SHAPES3 = [(8, 1024, 1024), (1, 4588, 4588), (1, 4589, 4589), (1, 2896, 2896), (1, 2897, 2897), (0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (65535, 64, 64),
                 (65536, 64, 64), (1, 1, 1), (2, 40, 72), (1, 1 << 20, 64), (1, 64, 1 << 20), ((1 << 40) + 1, 1, 1), (1 << 16, 974, 974), (1 << 21, 974, 974),
                 (3, 63, 65), (1, 1 << 16, 1 << 16), (4, 4096, 4096), (1, 8192, 2570), (1, 8192, 2571), (1, 5000, 4211), (1, 5000, 4210)]


def query_rows(name, names, argtypes):
    n = len(names)
    if n == 0:
        return [[]]
    if name == "sstem_status_string":
        return [[s] for s in range(-1, 8)]
    if names[:5] == ["N", "Cin", "H", "W", "Cout"]:
        last = {"algo": range(0, 8), "which": range(0, 5), "output_bf16": (0, 1)}.get(names[-1], ())
        tails = {5: [()], 6: [(a,) for a in last], 9: [(3, 3, t, a) for t in (0, 1) for a in (0, 1, 2)] + [(1, 1, 0, 2), (3, 5, 0, 0)]}[n]
        return [list(s) + list(t) for i, s in enumerate(QUERY_SHAPES5) for j, t in enumerate(tails) if i < 3 or j == i % len(tails)]
    if names[:2] == ["Cin", "Cout"]:
        pairs = [(64, 64), (6, 32), (51, 51), (512, 512), (3, 2), (1, 1), (0, 4), (4, 0), (-1, 4), (1 << 20, 1), ((1 << 20) + 1, 1), (1, (1 << 20) + 1), (16, 128)]
        tails = [()] if n == 2 else [(a,) for a in range(-1, 8)]
        rows = [list(p) + list(t) + ([HOST16] if n == 4 else []) for i, p in enumerate(pairs) for j, t in enumerate(tails)
                if i < 3 or j == i % len(tails)]
        return rows + ([[64, 64, a, None] for a in (2, 3, 99)] if n == 4 else [])
    if names == ["N", "H", "W", "Cout"]:
        return [[s[0], s[2], s[3], s[4]] for s in QUERY_SHAPES5] + [[65536, 8, 8, 6], [2, (1 << 20) + 1, 8, 6], [2, 8, (1 << 20) + 4, 6], [2, 1 << 15, 1 << 15, 6]]
    if names == ["N", "C", "HW"]:
        return [[2, 16, 64], [0, 16, 64], [-1, 16, 64], [(1 << 20) + 1, 1, 1], [1 << 20, 1, 1], [1, 65535, 1], [1, 65536, 1], [1, 1, 1 << 31], [1, 1, (1 << 31) + 1],
                [1 << 10, 1 << 10, 1 << 20], [1 << 10, 1 << 10, (1 << 20) - 1], [8, 64, 512 * 512], [32, 51, 1 << 20]]
    if names[:3] == ["B", "H", "W"]:
        return [list(s) + ([p] if n == 4 else []) for s in QUERY_SHAPES3 for p in ((3,) if n == 4 else (0,))]
    if names == ["B", "C", "H", "W"]:
        return [[s[0], 3, s[1], s[2]] for s in QUERY_SHAPES3[:14]]
    raise SystemExit("no query shapes for %s%r" % (name, names))


def main(path=os.path.join(HERE, "capi_refusals.json")):
    assert capi_replay.visible_devices() == 0, "run this where no device is visible (HIP_VISIBLE_DEVICES=-1)"
    lib = sstem_native.load_library()
    protos = prototypes()
    assert sorted(protos) == sorted(sstem_native.C_ABI)
    rows, dropped, messages, bases = [], 0, set(), {}
    for name in sorted(sstem_native.C_ABI):
        restype, argtypes = sstem_native.C_ABI[name]
        names = protos[name]
        assert len(names) == len(argtypes), name
        takes_tensors = any(t is _p and a != "stream" for a, t in zip(names, argtypes)) and name != "sstem_conv3x3_pack_group_entry"
        if name == "sstem_last_error":         # read after every refused call below; on its own it returns whatever came before
            continue
        if not takes_tensors:
            cases = [[None]] if names == ["stream"] else query_rows(name, names, argtypes)
            rows += [[name, a, call(lib, name, a)] for a in cases]
            continue
        base = base_args(name, names, argtypes)
        bases[name] = base
        muts, ptrs = mutations(names, argtypes, base)
        nulls = {a: None for a in ptrs}
        answers = {}                      # message -> the first mutation that gave it
        got_base = call(lib, name, base)
        assert got_base[0] == 4, "%s: the base call should pass validation, got %r" % (name, got_base)

        alike = {}                        # (arguments changed, answer) -> the rows with that answer, in probe order
        limited = set()                   # the argument sets of which some value is refused: the ones this entry has a rule on

        def record(mut, changed):
            nonlocal dropped
            args = apply(names, base, mut)
            got = call(lib, name, args)
            if got[0] in (4, 5) or (got[0] == 0 and any(args[names.index(a)] is not None for a in ptrs)):
                dropped += 1              # reached HIP, or an accepted call that holds a pointer: not for the file
                return None
            alike.setdefault((changed, str(got)), []).append([name, args, got])
            return got

        for m in muts:
            # one pointer null, whichever: one set.  A wrapper that only passes its arguments on takes the pointer and SHAPES cases
            changed = ("a pointer",) if all(a in ptrs for a in m) and len(m) == 1 else tuple(sorted(m))
            if name in WRAPPERS and len(m) == 1 and not all(a in ptrs for a in m):
                continue
            got = record(m, changed)
            if got and got[0] != 0:
                answers.setdefault(got[1], m)
                limited.add(changed)
            if got is None:                            # the side of a limit that passes: the same shape with every pointer null stops
                record({**m, **nulls}, changed + ("nulls",))   # at the null check (or is an accepted empty shape), not at a launch
        for (changed, _), same in alike.items():       # of the values that end alike, the first and the last (the lists ascend)
            if changed[-1] == "nulls" and changed[:-1] not in limited:      # no value of these arguments is refused here: nothing
                same = same[-1:] if len(changed) > 2 else []                # to pin for one argument, one row for a SHAPES case
            rows += [r for r in (same[:1] + same[-1:] if len(same) > 1 else same) if r not in rows]
        # two refusals at once: which one wins.  Every pair is tried; the wins order the checks, and the file keeps the pairs of
        # checks that are neighbours in that order
        pairs = []
        for (ma, a), (mb, b) in itertools.combinations(answers.items(), 2):
            if all(a[k] == b[k] for k in a if k in b):
                args = apply(names, base, {**a, **b})
                pairs.append((ma, mb, args, call(lib, name, args)))
        wins = {m: sum(1 for ma, mb, _, got in pairs if got[1] == m) for m in answers}
        order = sorted(answers, key=lambda m: -wins[m])
        for ma, mb, args, got in pairs:
            if abs(order.index(ma) - order.index(mb)) == 1 and got[0] not in (0, 4, 5) and [name, args, got] not in rows:
                rows.append([name, args, got])
        messages |= set(answers)
    for name, args, got in rows:
        restype, argtypes = sstem_native.C_ABI[name]
        if len(got) == 2 and not isinstance(got[1], list):
            assert got[0] not in (4, 5), (name, args, got)
            if got[0] == 0:
                assert all(a is None for a, t in zip(args, argtypes) if t is _p), (name, args, got)
            elif got[1]:
                messages.add(got[1])
    with open(path, "w") as f:
        dumps = lambda x: json.dumps(x, separators=(",", ":"))
        by_entry = {}                    # entry -> answer -> its calls, in the order they were made
        for name, args, got in rows:
            base = bases.get(name)
            if base:
                args = {a: v for a, v, b in zip(protos[name], args, base) if v != b or type(v) is not type(b)}
                ptrs = [a for a, t in zip(protos[name], sstem_native.C_ABI[name][1]) if t is _p and a != "stream"]
                if len(ptrs) > 1 and all(a in args and args[a] is None for a in ptrs):
                    args = {"pointers": None, **{a: v for a, v in args.items() if a not in ptrs}}
            calls = by_entry.setdefault(name, {}).setdefault(dumps(got), [])
            if dumps(args) not in calls:
                calls.append(dumps(args))
        entries = []
        for name, answers in by_entry.items():
            head = '"args":%s,"base":%s,' % (dumps(protos[name]), dumps(bases[name])) if name in bases else ""
            lines = ["[%s,[%s]]" % (got, ",".join(calls)) for got, calls in answers.items()]
            entries.append('"%s":{%s"answers":[\n%s]}' % (name, head, ",\n".join(lines)))
        f.write("{\n" + ",\n".join(entries) + "\n}\n")
    n_rows = sum(len(c) for answers in by_entry.values() for c in answers.values())
    print("wrote %d rows (%d distinct messages, %d calls dropped), %d bytes" % (n_rows, len(messages), dropped, os.path.getsize(path)))
    # every message literal of csrc/sstem_capi.hip against the file
    src = open(os.path.join(REPO, "sstem-restoration_amd", "csrc", "sstem_capi.hip")).read()
    lits = set()
    for m in re.finditer(r'\bfail\(\s*SSTEM_ERR_[A-Z_]+,\s*((?:"(?:[^"\\]|\\.)*"\s*)+)', src):
        lits.add("".join(re.findall(r'"((?:[^"\\]|\\.)*)"', m.group(1))))
    for lit in sorted(lits):
        pat = re.escape(lit.replace("%%", "%")).replace("%s", ".*")
        if not any(re.fullmatch(pat, msg) for msg in messages):
            print("no row for:", lit)


if __name__ == "__main__":
    main(*sys.argv[1:])
