"""CPU-side checks of the validation scores (include/sstem_score.h, utils/psnr_ssim.py, loss/multiscaleloss.py): the fixture and its
float64 yardstick, the exports, the workspace query and every refusal -- none of it needs a device."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scores_ref64 as R
import sstem_native

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_scores_golden as G  # noqa: E402


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "scores.npz"))


@pytest.mark.skipif(not G.reference_available(), reason="the reference tree is not on this machine")
def test_generator_reproduces_the_fixture(golden):
    fresh = G.generate()
    assert sorted(fresh) == sorted(golden.files)
    for k in golden.files:
        if "_dev_" in k:        # differences of nearly equal numbers: the same size, not the same bits, on another host
            assert np.all(fresh[k] <= 2 * golden[k] + 1e-12), k
        elif k.endswith(("_a", "_b", "_flow", "_target")):
            assert np.array_equal(fresh[k], golden[k]), k
        else:                   # the reference's results: its own rounding noise apart (another numpy / BLAS / thread count)
            assert np.allclose(fresh[k], golden[k], rtol=1e-6, atol=0, equal_nan=True), k


def test_inputs_follow_the_recipe(golden):
    for name, (kind, H, W) in R.IMAGE_CASES.items():
        a, b = R.make_image_case(name)
        assert np.array_equal(a, golden[name + "_a"]) and np.array_equal(b, golden[name + "_b"])
        assert a.shape == (H, W) and a.dtype == (np.uint8 if kind in ("u8", "bits") else np.float32)
        if kind in ("f32", "u8", "bits"):
            assert 0.3 < float(golden[name + "_ssim"]) < 0.9, name           # neither near 0 nor near 1
    assert float(golden["same_ssim"]) == 1.0 and float(golden["same_psnr"]) == 1e12 and np.isnan(golden["same_mse"])
    a, b = golden["over1_a"], golden["over1_b"]
    assert a.max() == 1.5 and (a > 1).sum() == 1 and b.max() <= 1            # one value selects the other branch
    assert golden["u43x44_a"].max() > 1 and set(np.unique(golden["bits_a"])) == {0, 1} and (golden["bits_a"] != golden["bits_b"]).any()
    for name, (shape, kind) in R.FLOW_CASES.items():
        flow, target = R.make_flow_case(name)
        assert np.array_equal(flow, golden[name + "_flow"]) and np.array_equal(target, golden[name + "_target"]) and flow.shape == shape
        holes = int(((target[:, 0] == 0) & (target[:, 1] == 0)).sum())
        assert {"dense": holes == 0, "holes": 0 < holes < target[:, 0].size, "empty": holes == target[:, 0].size}[kind]
    assert np.isnan(golden["small_empty_epe"][1, 1]) and golden["small_empty_epe"][1, 0] == 0


def test_ref64_ssim_equals_the_reference(golden):
    for name in R.IMAGE_CASES:
        a, b = torch.from_numpy(golden[name + "_a"]), torch.from_numpy(golden[name + "_b"])
        assert abs(R.ssim64(a, b) - float(golden[name + "_ssim"])) <= 1e-12, name
        assert float(golden[name + "_dev_ssim"]) <= 1e-12


def test_ref64_psnr_and_epe_within_the_recorded_deviations(golden):
    slack = 1.0 + 1e-6
    for name in R.IMAGE_CASES:
        a, b = torch.from_numpy(golden[name + "_a"]), torch.from_numpy(golden[name + "_b"])
        mse, psnr = R.psnr64(a, b)
        if name == "same":
            assert mse == 0.0 and psnr == 1e12
            continue
        assert abs(float(golden[name + "_mse"]) - mse) <= float(golden[name + "_dev_mse"]) * mse * slack + 1e-18, name
        assert abs(float(golden[name + "_psnr"]) - psnr) <= float(golden[name + "_dev_psnr"]) * slack + 1e-12, name
        # the recorded deviations are fp32 rounding (float32 arrays) or nothing (bytes: the reference is float64 there)
        assert float(golden[name + "_dev_mse"]) < (1e-12 if a.dtype == torch.uint8 else 1e-6), name
    for name in R.FLOW_CASES:
        f, t = torch.from_numpy(golden[name + "_flow"]), torch.from_numpy(golden[name + "_target"])
        for sparse in (0, 1):
            for mean in (0, 1):
                want, dev = float(golden[name + "_epe"][sparse, mean]), float(golden[name + "_dev_epe"][sparse, mean])
                v = R.epe64(f, t, bool(sparse), bool(mean))
                if np.isnan(want):
                    assert np.isnan(v) and (name, sparse, mean) == ("small_empty", 1, 1)
                    continue
                assert abs(want - v) <= dev * abs(v) * slack + 1e-12, (name, sparse, mean)
                assert dev < 1e-6


def test_window_is_the_outer_product_of_the_normalised_taps():
    """What the kernels rely on: the reference's 2-D window, its eps cut (which zeroes nothing at sigma 1.5) and its two
    normalisations are the outer product of the 11 normalised taps."""
    g = torch.exp(-torch.arange(-5, 6, dtype=torch.float64) ** 2 / (2 * 1.5 * 1.5))
    g = g / g.sum()
    w = R.window2d()
    assert float(w.min()) > 0 and float((w - torch.outer(g, g)).abs().max()) <= 1e-17


def test_library_exports_the_four_entries():
    lib = ctypes.CDLL(sstem_native.library_path())
    for name in ("sstem_score_workspace_bytes", "sstem_score_images_f32", "sstem_score_images_u8", "sstem_flow_epe_f32"):
        assert hasattr(lib, name) and name in sstem_native.C_ABI


def test_workspace_query():
    q = sstem_native.load_library().sstem_score_workspace_bytes
    sizes = [(1, 11, 11), (2, 11, 11), (2, 43, 44), (3, 75, 53), (16, 256, 256), (16, 1024, 1024)]
    got = [q(B, H, W) for B, H, W in sizes]
    assert all(g > 0 and g % 8 == 0 for g in got)
    assert got == sorted(got) and len(set(got)) == len(got)
    assert q(3, 7, 9) > 0 and q(0, 64, 64) > 0            # the end-point error has no 11 x 11 floor; an empty batch needs nothing more
    # sizes the entries refuse
    assert q(-1, 64, 64) == 0 and q(1, -1, 64) == 0 and q(1, 64, -1) == 0
    assert q(1, (1 << 15) + 1, 64) == 0 and q(1, 64, (1 << 15) + 1) == 0 and q((1 << 24) + 1, 11, 11) == 0
    assert q(1 << 24, 43, 11) == 0                        # more than 2^24 tiles


# (status, text of sstem_last_error) per refusal; P = a non-null "pointer" that is never dereferenced: every row is refused (or is the
# empty no-op) before any HIP call, which the child process below proves by running without a device
_P = 64
_RANGE = "sizes past the index range (H, W <= 32768, B <= 2^24, at most 2^24 tiles of 32 x 16)"
_SMALL = "H and W must be at least 11 (the 'valid' map of the 11 x 11 window would be empty)"
_ROWS = []
for _entry, _what in (("sstem_score_images_f32", "score images (f32)"), ("sstem_score_images_u8", "score images (u8)")):
    _ROWS += [
        # entry, (a, b, B, H, W, clamp01_a, scores, workspace), expected status, expected message
        (_entry, (None, _P, 1, 32, 32, 0, _P, _P), 1, _what + ": null pointer"),
        (_entry, (_P, None, 1, 32, 32, 0, _P, _P), 1, _what + ": null pointer"),
        (_entry, (_P, _P, 1, 32, 32, 1, None, _P), 1, _what + ": null pointer"),
        (_entry, (_P, _P, 1, 32, 32, 0, _P, None), 1, _what + ": null pointer"),
        (_entry, (_P, _P, -1, 32, 32, 0, _P, _P), 2, _what + ": negative size"),
        (_entry, (_P, _P, 1, -32, 32, 0, _P, _P), 2, _what + ": negative size"),
        (_entry, (_P, _P, 1, 32, -32, 0, _P, _P), 2, _what + ": negative size"),
        (_entry, (_P, _P, 1, 10, 32, 0, _P, _P), 2, _what + ": " + _SMALL),
        (_entry, (_P, _P, 1, 32, 10, 0, _P, _P), 2, _what + ": " + _SMALL),
        (_entry, (_P, _P, 1, 0, 0, 0, _P, _P), 2, _what + ": " + _SMALL),
        (_entry, (_P, _P, 1, (1 << 15) + 1, 32, 0, _P, _P), 3, _what + ": " + _RANGE),
        (_entry, (_P, _P, (1 << 24) + 1, 32, 32, 0, _P, _P), 3, _what + ": " + _RANGE),
        (_entry, (_P, _P, 1 << 24, 43, 11, 0, _P, _P), 3, _what + ": " + _RANGE),
        (_entry, (_P, _P, 1, 32, 32, 0, _P, _P + 4), 3, _what + ": the workspace and the result must be 8-byte aligned"),
        (_entry, (_P, _P, 1, 32, 32, 0, _P + 4, _P), 3, _what + ": the workspace and the result must be 8-byte aligned"),
        # B == 0: a successful no-op, whatever the pointers
        (_entry, (None, None, 0, 32, 32, 0, None, None), 0, None),
        (_entry, (None, None, 0, 3, 3, 1, None, None), 0, None),
    ]
_ROWS += [
    # (flow, target, B, H, W, sparse, mean, value, workspace)
    ("sstem_flow_epe_f32", (None, _P, 1, 7, 9, 0, 1, _P, _P), 1, "flow epe: null pointer"),
    ("sstem_flow_epe_f32", (_P, None, 1, 7, 9, 0, 1, _P, _P), 1, "flow epe: null pointer"),
    ("sstem_flow_epe_f32", (_P, _P, 1, 7, 9, 1, 1, None, _P), 1, "flow epe: null pointer"),
    ("sstem_flow_epe_f32", (_P, _P, 1, 7, 9, 1, 0, _P, None), 1, "flow epe: null pointer"),
    ("sstem_flow_epe_f32", (_P, _P, -1, 7, 9, 0, 1, _P, _P), 2, "flow epe: negative size"),
    ("sstem_flow_epe_f32", (_P, _P, 1, -7, 9, 0, 1, _P, _P), 2, "flow epe: negative size"),
    ("sstem_flow_epe_f32", (_P, _P, 1, 7, -9, 0, 1, _P, _P), 2, "flow epe: negative size"),
    ("sstem_flow_epe_f32", (_P, _P, 1, 7, (1 << 15) + 1, 0, 1, _P, _P), 3, "flow epe: " + _RANGE),
    ("sstem_flow_epe_f32", (_P, _P, (1 << 24) + 1, 7, 9, 0, 1, _P, _P), 3, "flow epe: " + _RANGE),
    ("sstem_flow_epe_f32", (_P, _P, 1, 7, 9, 0, 1, _P + 4, _P), 3, "flow epe: the workspace and the result must be 8-byte aligned"),
    ("sstem_flow_epe_f32", (None, None, 0, 7, 9, 0, 1, None, None), 0, None),
]

_CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
import sstem_native
lib = sstem_native.load_library()
path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
n = ctypes.c_int(0)
rc = ctypes.CDLL(path).hipGetDeviceCount(ctypes.byref(n))
if rc == 0 and n.value > 0:
    print("DEVICE"); sys.exit(77)
out = []
for name, args in json.loads(sys.argv[2]):
    rc = getattr(lib, name)(*args, None)
    out.append([rc, lib.sstem_last_error().decode() if rc else None])
print("ANSWERS " + json.dumps(out))
"""


def test_every_refusal_fires_without_a_device(repo_root):
    rows = [[name, list(args)] for name, args, _, _ in _ROWS]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(repo_root, "sstem-restoration_amd"), json.dumps(rows)], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode == 77:
        pytest.skip("the child process sees a device despite HIP_VISIBLE_DEVICES=-1: nothing replayed")
    assert p.returncode == 0, p.stdout[-3000:]
    answers = json.loads(next(line for line in p.stdout.splitlines() if line.startswith("ANSWERS "))[8:])
    assert len(answers) == len(_ROWS)
    for (name, args, status, text), got in zip(_ROWS, answers):
        assert got == [status, text], (name, args, got)      # status 4 / 5 here would mean a call got past its checks to HIP


def test_python_layer_refuses_cpu_input_and_other_shapes():
    from loss.multiscaleloss import EPE, realEPE
    from utils.psnr_ssim import compute_psnr, compute_ssim, score_batch
    img = torch.zeros(16, 16)
    for fn in (compute_psnr, compute_ssim):
        with pytest.raises(NotImplementedError):
            fn(img, img)
        with pytest.raises(NotImplementedError):
            fn(img.numpy(), img.numpy())
    with pytest.raises(NotImplementedError):
        score_batch(img[None], img[None])
    with pytest.raises(NotImplementedError):
        score_batch(img[None].numpy(), img[None].numpy(), clamp01=True)
    flow = torch.zeros(1, 2, 7, 9)
    with pytest.raises(NotImplementedError):
        EPE(flow, flow)
    with pytest.raises(NotImplementedError):
        realEPE(flow, flow, sparse=True)
    with pytest.raises(NotImplementedError, match="up-sampling"):
        realEPE(torch.zeros(1, 2, 4, 5), flow)


def test_the_modules_hold_no_torch_or_numpy_formulation(repo_root):
    """utils/psnr_ssim.py scores through the library only: no convolution, no reduction and no numpy in it."""
    text = open(os.path.join(repo_root, "sstem-restoration_amd", "utils", "psnr_ssim.py")).read()
    code = text.split('"""', 2)[2]
    for word in ("import numpy", "conv2d", ".mean(", ".sum(", "log10", ".max("):
        assert word not in code, word


def test_steps_have_the_validation_pass():
    import steps
    assert callable(steps.FusionStep.validate) and callable(steps.IFNetStep.validate)
    assert not hasattr(steps.SPJointStep, "validate")
