"""CPU-side checks of the MS-SSIM criterion (include/sstem_loss.h, loss/loss_ssim.py): the fixture and its float64 yardsticks, the
exports, the workspace query and every refusal -- none of it needs a device."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ms_ssim_ref64 as R
import sstem_native

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_ms_ssim_golden as G  # noqa: E402


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "ms_ssim.npz"))


@pytest.mark.skipif(not G.reference_available(), reason="the reference tree is not on this machine")
def test_generator_reproduces_the_fixture(golden):
    fresh = G.generate()
    assert sorted(fresh) == sorted(golden.files)
    for k in golden.files:
        if "_dev_" in k:        # differences of nearly equal numbers: the same size, not the same bits, on another host
            assert fresh[k] <= 2 * golden[k] + 1e-9, k
        elif k.endswith(("_pred", "_target", "_max_val")):
            assert np.array_equal(fresh[k], golden[k]), k
        else:                   # the reference's fp32 results: its own rounding noise apart (another BLAS / thread count)
            scale = np.abs(golden[k]).max()
            assert np.abs(fresh[k].astype(np.float64) - golden[k]).max() <= 1e-5 * scale, k


def test_inputs_follow_the_recipe(golden):
    for i, ((B, H, W), max_val) in enumerate(R.CASES):
        pred, target = R.make_pair(B, H, W, R.case_seed(i), scale=max_val)
        assert np.array_equal(pred, golden["c%d_pred" % i]) and np.array_equal(target, golden["c%d_target" % i])
        assert pred.shape == (B, 1, H, W) and float(golden["c%d_max_val" % i]) == max_val
        mcs = golden["c%d_terms" % i][:, 1]
        assert (mcs > 0.85).all() and (mcs < 0.9995).all(), mcs         # no level is ill-conditioned, none a constant 1


def test_ref64_matches_the_golden_within_the_recorded_deviations(golden):
    for i, (_, max_val) in enumerate(R.CASES):
        k = "c%d_" % i
        pred, target = torch.from_numpy(golden[k + "pred"]), torch.from_numpy(golden[k + "target"])
        v, t, g = R.ref64(pred, target, max_val, 5)
        slack = 1.0 + 1e-6
        assert abs(float(golden[k + "value"]) - float(v)) <= float(golden[k + "dev_value"]) * slack + 1e-12
        assert np.abs(golden[k + "terms"].astype(np.float64) - t.numpy()).max() <= float(golden[k + "dev_terms"]) * slack + 1e-12
        gmax = float(g.abs().max())
        assert np.abs(golden[k + "grad"].astype(np.float64) - g.numpy()).max() / gmax <= float(golden[k + "dev_grad"]) * slack + 1e-12
        # the recorded deviations are fp32 rounding, not a different function
        assert float(golden[k + "dev_value"]) < 5e-6 and float(golden[k + "dev_grad"]) < 5e-5


@pytest.mark.parametrize("levels", [1, 2, 5])
def test_manual64_matches_ref64_autograd(golden, levels):
    """The kernels' formulas (separable taps, adjoint blur, gather from the coarser level, coefficients) against autograd through the
    reference's formulation: 1e-5 of the gradient's max-norm (observed 1e-6: the fp32 2-D window against separable taps)."""
    for i, (_, max_val) in enumerate(R.CASES):
        k = "c%d_" % i
        pred, target = torch.from_numpy(golden[k + "pred"]), torch.from_numpy(golden[k + "target"])
        v, t, g = R.ref64(pred, target, max_val, levels)
        v2, t2, g2 = R.manual64(pred, target, max_val, levels)
        assert abs(float(v) - float(v2)) <= 1e-6
        assert float((t[:levels] - t2).abs().max()) <= 1e-6
        assert float((g - g2).abs().max()) <= 1e-5 * float(g.abs().max())


def test_library_exports_the_three_entries():
    lib = ctypes.CDLL(sstem_native.library_path())
    for name in ("sstem_ms_ssim_workspace_floats", "sstem_ms_ssim_forward_f32", "sstem_ms_ssim_backward_f32"):
        assert hasattr(lib, name) and name in sstem_native.C_ABI


def test_workspace_query_is_positive_and_monotone():
    lib = sstem_native.load_library()
    q = lib.sstem_ms_ssim_workspace_floats
    sizes = [(1, 32, 32), (2, 32, 32), (2, 37, 70), (3, 64, 48), (2, 256, 256), (16, 256, 256), (16, 512, 512)]
    got = [q(B, H, W, 5) for B, H, W in sizes]
    assert all(g > 0 for g in got)
    assert got == sorted(got) and len(set(got)) == len(got)
    assert q(2, 64, 64, 1) < q(2, 64, 64, 2) < q(2, 64, 64, 5)          # no pyramid to keep for one level
    # sizes the entries refuse
    assert q(2, 31, 64, 5) == 0 and q(2, 64, 31, 5) == 0 and q(2, 16, 16, 4) > 0
    assert q(2, 64, 64, 0) == 0 and q(2, 64, 64, 6) == 0 and q(-1, 64, 64, 5) == 0
    assert q(1, 1 << 16, 64, 5) == 0 and q(1 << 25, 32, 32, 5) == 0


# (status, text of sstem_last_error) per refusal; P = a non-null "pointer" that is never dereferenced: every row is refused (or is the
# empty no-op) before any HIP call, which the child process below proves by running without a device
_P = 64
_ROWS = [
    # name, args after (img1, img2), expected status, expected message
    ("forward", (None, _P, 1, 32, 32, 5, 1.0, _P, None, _P), 1, "ms_ssim forward: null pointer"),
    ("forward", (_P, None, 1, 32, 32, 5, 1.0, _P, None, _P), 1, "ms_ssim forward: null pointer"),
    ("forward", (_P, _P, 1, 32, 32, 5, 1.0, None, None, _P), 1, "ms_ssim forward: null pointer"),
    ("forward", (_P, _P, 1, 32, 32, 5, 1.0, _P, None, None), 1, "ms_ssim forward: null pointer"),
    ("backward", (None, _P, 1, 32, 32, 5, 1.0, None, _P, _P), 1, "ms_ssim backward: null pointer"),
    ("backward", (_P, _P, 1, 32, 32, 5, 1.0, None, None, _P), 1, "ms_ssim backward: null pointer"),
    ("backward", (_P, _P, 1, 32, 32, 5, 1.0, None, _P, None), 1, "ms_ssim backward: null pointer"),
    ("forward", (_P, _P, 1, 32, 32, 0, 1.0, _P, None, _P), 3, "ms_ssim forward: levels must be 1..5"),
    ("forward", (_P, _P, 1, 32, 32, 6, 1.0, _P, None, _P), 3, "ms_ssim forward: levels must be 1..5"),
    ("backward", (_P, _P, 1, 32, 32, 6, 1.0, None, _P, _P), 3, "ms_ssim backward: levels must be 1..5"),
    ("forward", (_P, _P, 1, 31, 32, 5, 1.0, _P, None, _P), 2,
     "ms_ssim forward: min(H, W) must be at least 2^levels (every level is pooled 2 x 2 once more)"),
    ("forward", (_P, _P, 1, 64, 3, 2, 1.0, _P, None, _P), 2,
     "ms_ssim forward: min(H, W) must be at least 2^levels (every level is pooled 2 x 2 once more)"),
    ("backward", (_P, _P, 1, 32, 31, 5, 1.0, None, _P, _P), 2,
     "ms_ssim backward: min(H, W) must be at least 2^levels (every level is pooled 2 x 2 once more)"),
    ("forward", (_P, _P, 1, 32, 32, 5, 0.0, _P, None, _P), 3, "ms_ssim forward: max_val must be positive and finite"),
    ("forward", (_P, _P, 1, 32, 32, 5, -1.0, _P, None, _P), 3, "ms_ssim forward: max_val must be positive and finite"),
    ("forward", (_P, _P, 1, 32, 32, 5, float("nan"), _P, None, _P), 3, "ms_ssim forward: max_val must be positive and finite"),
    ("backward", (_P, _P, 1, 32, 32, 5, float("inf"), None, _P, _P), 3, "ms_ssim backward: max_val must be positive and finite"),
    ("forward", (_P, _P, 1, 1 << 16, 32, 5, 1.0, _P, None, _P), 3,
     "ms_ssim forward: sizes past the index range (H, W <= 32768 and at most 2^24 tiles of 32 x 32)"),
    ("backward", (_P, _P, 1 << 25, 32, 32, 5, 1.0, None, _P, _P), 3,
     "ms_ssim backward: sizes past the index range (H, W <= 32768 and at most 2^24 tiles of 32 x 32)"),
    ("forward", (_P, _P, -1, 32, 32, 5, 1.0, _P, None, _P), 2, "ms_ssim forward: negative size"),
    ("forward", (_P, _P, 1, 32, 32, 5, 1.0, _P, None, _P + 4), 3, "ms_ssim forward: the workspace must be 8-byte aligned"),
    # B == 0: a successful no-op, whatever the pointers
    ("forward", (None, None, 0, 32, 32, 5, 1.0, None, None, None), 0, None),
    ("backward", (None, None, 0, 32, 32, 5, 1.0, None, None, None), 0, None),
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
    args = [float(a[1]) if isinstance(a, list) else a for a in args]
    rc = getattr(lib, "sstem_ms_ssim_%s_f32" % name)(*args, None)
    out.append([rc, lib.sstem_last_error().decode() if rc else None])
print("ANSWERS " + json.dumps(out))
"""


def test_every_refusal_fires_without_a_device(repo_root):
    import json
    rows = [[name, [["f", repr(a)] if isinstance(a, float) else a for a in args]] for name, args, _, _ in _ROWS]
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


def test_python_layer_refuses_cpu_tensors_and_other_shapes():
    from loss.loss_ssim import MS_SSIM
    crit = MS_SSIM(max_val=1)
    assert crit.max_val == 1 and crit.size_average is True and crit.channel == 1
    assert MS_SSIM().max_val == 255
    with pytest.raises(NotImplementedError):
        crit(torch.zeros(1, 1, 32, 32), torch.zeros(1, 1, 32, 32))
    import train_utils
    with pytest.raises(NotImplementedError):
        train_utils.MSSSIMLoss("cpu")(torch.zeros(1, 1, 32, 32), torch.zeros(1, 1, 32, 32))


def test_fusion_step_rejects_an_unknown_loss_name():
    import steps
    with pytest.raises(AttributeError, match="No this loss function!"):
        steps.FusionStep("cpu", loss="L2")          # refused before any module is built or moved to a device


def test_torch_formulation_is_the_same_function(golden):
    """loss.loss_ssim.ms_ssim_torch (the SSTEM_NATIVE_SSIM=0 path) in float64 against ref64: the same function, value and gradient."""
    from loss.loss_ssim import ms_ssim_torch
    for i in (1, 6):
        k = "c%d_" % i
        max_val = float(golden[k + "max_val"])
        pred = torch.from_numpy(golden[k + "pred"]).double().requires_grad_(True)
        target = torch.from_numpy(golden[k + "target"]).double()
        v = ms_ssim_torch(pred, target, max_val)
        v.backward()
        v64, _, g64 = R.ref64(pred, target, max_val, 5)
        assert abs(float(v.detach()) - float(v64)) <= 1e-12
        assert float((pred.grad - g64).abs().max()) <= 1e-10 * float(g64.abs().max())
