"""CPU-side checks of the single-scale SSIM criterion (include/sstem_loss.h, loss/loss_ssim.py: SSIMLoss, ssim): the fixture and its
float64 yardsticks, mutants of the kernels' formulas, the exports, the workspace query and every refusal -- none of it needs a device."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ssim_loss_ref64 as R
import sstem_native

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_ssim_loss_golden as G  # noqa: E402

# the ceilings tests/test_ms_ssim_cpu.py asserts on the recorded deviations, and its allowance for manual64 against ref64
DEV_VALUE_CEILING, DEV_GRAD_CEILING, MANUAL_REL = 5e-6, 5e-5, 1e-5


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "ssim_loss.npz"))


def _case(golden, i):
    k = "c%d_" % i
    return torch.from_numpy(golden[k + "pred"]), torch.from_numpy(golden[k + "target"]), bool(golden[k + "size_average"])


@pytest.mark.skipif(not G.reference_available(), reason="the reference tree is not on this machine")
def test_generator_reproduces_the_fixture(golden):
    fresh = G.generate()
    assert sorted(fresh) == sorted(golden.files)
    for k in golden.files:
        if "_dev_" in k:        # differences of nearly equal numbers: the same size, not the same bits, on another host
            assert fresh[k] <= 2 * golden[k] + 1e-9, k
        elif k.endswith(("_pred", "_target", "_size_average")):
            assert np.array_equal(fresh[k], golden[k]), k
        else:                   # the reference's fp32 results: its own rounding noise apart (another BLAS / thread count)
            scale = np.abs(golden[k]).max()
            assert np.abs(fresh[k].astype(np.float64) - golden[k]).max() <= 1e-5 * scale, k


def test_inputs_follow_the_recipe(golden, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "ssim_loss.npz")) < os.path.getsize(os.path.join(golden_dir, "ms_ssim.npz"))
    assert [shape for shape, _ in R.CASES[:6]] == [(1, 1, 5, 7), (1, 1, 11, 11), (2, 1, 33, 31), (2, 3, 45, 70), (1, 1, 96, 80), (3, 1, 20, 40)]
    assert [sa for _, sa in R.CASES] == [True] * 5 + [False, True]
    for i, (shape, size_average) in enumerate(R.CASES):
        pred, target = R.make_case(i)
        k = "c%d_" % i
        assert np.array_equal(pred, golden[k + "pred"]) and np.array_equal(target, golden[k + "target"])
        assert pred.shape == shape and pred.dtype == np.float32 and bool(golden[k + "size_average"]) == size_average
        assert pred.min() >= 0.0 and pred.max() <= 1.0 and target.min() >= 0.0 and target.max() <= 1.0
        assert golden[k + "value"].shape == (() if size_average else (shape[0],)) and golden[k + "grad"].shape == shape
        assert np.isfinite(golden[k + "value"]).all() and np.isfinite(golden[k + "grad"]).all()
    pred, target = R.make_case(R.CONSTANT_CASE)
    assert np.ptp(pred) == 0 and np.ptp(target) == 0 and pred[0, 0, 0, 0] != target[0, 0, 0, 0]


def test_ref64_matches_the_golden_within_the_recorded_deviations(golden):
    for i in range(len(R.CASES)):
        k = "c%d_" % i
        pred, target, size_average = _case(golden, i)
        v, g = R.ref64(pred, target, size_average)
        slack = 1.0 + 1e-6
        assert np.abs(golden[k + "value"].astype(np.float64) - v.numpy()).max() <= float(golden[k + "dev_value"]) * slack + 1e-12
        gmax = float(g.abs().max())
        assert np.abs(golden[k + "grad"].astype(np.float64) - g.numpy()).max() / gmax <= float(golden[k + "dev_grad"]) * slack + 1e-12
        # the recorded deviations are fp32 rounding, not a different function
        assert float(golden[k + "dev_value"]) < DEV_VALUE_CEILING and float(golden[k + "dev_grad"]) < DEV_GRAD_CEILING


def test_manual64_matches_ref64_autograd(golden):
    """The kernels' formulas (separable taps, the map's derivatives, the second blur, -grad / N) against autograd through the
    reference's formulation: 1e-5 of the gradient's max-norm (the fp32 2-D window against separable taps)."""
    for i in range(len(R.CASES)):
        pred, target, size_average = _case(golden, i)
        for gv in (None, torch.tensor(0.5)) + ((torch.tensor([0.5, -2.0, 3.0]),) if not size_average else ()):
            v, g = R.ref64(pred, target, size_average, grad_value=gv)
            v2, g2 = R.manual64(pred, target, size_average, grad_value=gv)
            assert float((v - v2).abs().max()) <= 1e-6
            assert float((g - g2).abs().max()) <= MANUAL_REL * float(g.abs().max())
        # the other image's gradient: the same formulas with the operands exchanged
        _, _, g_other = R.ref64(pred, target, size_average, want_grad2=True)
        _, g2 = R.manual64(target, pred, size_average)
        assert float((g_other - g2).abs().max()) <= MANUAL_REL * float(g_other.abs().max())


def _fixture_check(golden, fn):
    """fn(pred, target, size_average) -> value, grad against the reference's recorded fp32 numbers: within the ceilings on the
    reference's own deviation plus manual64's allowance.  -> the cases that fail."""
    bad = []
    for i in range(len(R.CASES)):
        k = "c%d_" % i
        pred, target, size_average = _case(golden, i)
        v, g = fn(pred, target, size_average)
        gold_g = torch.from_numpy(golden[k + "grad"]).double()
        dv = float((torch.as_tensor(golden[k + "value"]).double() - v).abs().max())
        dg = float((gold_g - g).abs().max()) / float(gold_g.abs().max())
        if dv > DEV_VALUE_CEILING + 1e-6 or dg > DEV_GRAD_CEILING + MANUAL_REL:
            bad.append(i)
    return bad


def test_manual64_passes_the_fixture_check_and_every_mutant_fails_it(golden):
    assert _fixture_check(golden, R.manual64) == []
    assert len(R.MUTANTS) >= 4
    failing = {m: _fixture_check(golden, lambda p, t, sa, m=m: R.manual64(p, t, sa, mutant=m)) for m in R.MUTANTS}
    assert all(failing.values()), failing
    assert failing["shrunk_window"] == [0]                    # the one image narrower than the window
    assert failing["batch_mean"] == [5]                       # the one per-sample case
    assert len(failing["max_val"]) == len(R.CASES) and len(failing["dropped_x_blur_b"]) == len(R.CASES)


def test_torch_formulation_is_the_same_function(golden):
    """loss.loss_ssim.ssim_loss_torch (the SSTEM_NATIVE_SSIM=0 path of the interpolation step) in float64 against ref64."""
    from loss.loss_ssim import ssim_loss_torch
    for i in (0, 3, 5):
        pred, target, size_average = _case(golden, i)
        a = pred.double().requires_grad_(True)
        b = target.double().requires_grad_(True)
        v = ssim_loss_torch(a, b, size_average)
        v.sum().backward()
        v64, g1, g2 = R.ref64(pred, target, size_average, want_grad2=True)
        assert float((v.detach() - v64).abs().max()) <= 1e-12
        assert float((a.grad - g1).abs().max()) <= 1e-10 * float(g1.abs().max())
        assert float((b.grad - g2).abs().max()) <= 1e-10 * float(g2.abs().max())


def test_window_helpers():
    from loss.loss_ssim import create_window, gaussian
    assert torch.equal(gaussian(11, 1.5), R.taps32())
    w = create_window(11, 3)
    assert w.shape == (3, 1, 11, 11) and w.dtype == torch.float32 and w.is_contiguous()
    assert torch.equal(w, R.window32(3))
    assert abs(float(gaussian(5, 1.5).sum()) - 1.0) < 1e-6


def test_the_reference_scripts_import_line_works():
    """``from loss.loss_ssim import SSIMLoss`` (sff_scripts_interp/main_ms.py:27) next to the fusion loop's MS_SSIM."""
    from loss.loss_ssim import SSIMLoss, ssim, MS_SSIM  # noqa: F401
    crit = SSIMLoss()
    assert isinstance(crit, torch.nn.Module)
    assert crit.window_size == 11 and crit.size_average is True and crit.channel == 1 and crit.window.shape == (1, 1, 11, 11)
    assert SSIMLoss(size_average=False).size_average is False


def test_library_exports_the_entries():
    lib = ctypes.CDLL(sstem_native.library_path())
    for name in ("sstem_ssim_loss_workspace_floats", "sstem_ssim_loss_forward_f32", "sstem_ssim_loss_backward_f32",
                 "sstem_l2_mean_forward_grad_f32"):
        assert hasattr(lib, name) and name in sstem_native.C_ABI


def test_workspace_query():
    lib = sstem_native.load_library()
    q = lib.sstem_ssim_loss_workspace_floats
    # a 64-byte header and one double per 32 x 32 tile of every plane
    assert q(1, 1, 5, 7) == 16 + 2 and q(1, 1, 32, 32) == 16 + 2 and q(1, 1, 33, 32) == 16 + 4 and q(2, 3, 45, 70) == 16 + 2 * 6 * 6
    sizes = [(1, 1, 5, 7), (2, 1, 33, 31), (2, 3, 45, 70), (8, 1, 256, 256), (1, 1, 1024, 1024), (16, 3, 1024, 1024)]
    got = [q(*s) for s in sizes]
    assert got == sorted(got) and len(set(got)) == len(got)
    assert q(8, 1, 256, 256) % 2 == 0
    # empty shapes and sizes the entries refuse
    assert q(0, 1, 8, 8) == 0 and q(1, 0, 8, 8) == 0 and q(1, 1, 0, 8) == 0 and q(1, 1, 8, 0) == 0
    assert q(-1, 1, 8, 8) == 0 and q(1, -1, 8, 8) == 0 and q(1, 1, -8, 8) == 0
    assert q(1, 1, 1 << 15, 8) > 0 and q(1, 1, (1 << 15) + 1, 8) == 0 and q(1, 1, 8, (1 << 15) + 1) == 0
    assert q(1 << 24, 1, 8, 8) > 0 and q((1 << 24) + 1, 1, 8, 8) == 0 and q(1 << 13, 1 << 12, 8, 8) == 0 and q(1 << 24, 1, 33, 8) == 0


# (status, text of sstem_last_error) per refusal; P = a non-null "pointer" that is never dereferenced: every row is refused (or is the
# empty no-op) before any HIP call, which the child process below proves by running without a device
_P = 64
_RANGE = "sizes past the index range (H, W <= 32768 and at most 2^24 tiles of 32 x 32)"
_ROWS = [
    # entry, args before the stream, expected status, expected message
    ("ssim_loss_forward", (None, _P, 1, 1, 16, 16, 0, _P, _P), 1, "ssim_loss forward: null pointer"),
    ("ssim_loss_forward", (_P, None, 1, 1, 16, 16, 0, _P, _P), 1, "ssim_loss forward: null pointer"),
    ("ssim_loss_forward", (_P, _P, 1, 1, 16, 16, 1, None, _P), 1, "ssim_loss forward: null pointer"),
    ("ssim_loss_forward", (_P, _P, 1, 1, 16, 16, 0, _P, None), 1, "ssim_loss forward: null pointer"),
    ("ssim_loss_backward", (None, _P, 1, 1, 16, 16, 0, None, _P, _P), 1, "ssim_loss backward: null pointer"),
    ("ssim_loss_backward", (_P, None, 1, 1, 16, 16, 0, _P, _P, _P), 1, "ssim_loss backward: null pointer"),
    ("ssim_loss_backward", (_P, _P, 1, 1, 16, 16, 1, None, None, _P), 1, "ssim_loss backward: null pointer"),
    ("ssim_loss_backward", (_P, _P, 1, 1, 16, 16, 0, None, _P, None), 1, "ssim_loss backward: null pointer"),
    ("ssim_loss_forward", (_P, _P, -1, 1, 16, 16, 0, _P, _P), 2, "ssim_loss forward: negative size"),
    ("ssim_loss_forward", (_P, _P, 1, -1, 16, 16, 0, _P, _P), 2, "ssim_loss forward: negative size"),
    ("ssim_loss_forward", (_P, _P, 1, 1, -16, 16, 0, _P, _P), 2, "ssim_loss forward: negative size"),
    ("ssim_loss_backward", (_P, _P, 1, 1, 16, -16, 0, None, _P, _P), 2, "ssim_loss backward: negative size"),
    ("ssim_loss_backward", (_P, _P, 0, -1, 16, 16, 0, None, _P, _P), 2, "ssim_loss backward: negative size"),
    ("ssim_loss_forward", (_P, _P, 1, 1, (1 << 15) + 1, 16, 0, _P, _P), 3, "ssim_loss forward: " + _RANGE),
    ("ssim_loss_forward", (_P, _P, 1, 1, 16, 1 << 16, 0, _P, _P), 3, "ssim_loss forward: " + _RANGE),
    ("ssim_loss_forward", (_P, _P, 1 << 13, 1 << 12, 16, 16, 0, _P, _P), 3, "ssim_loss forward: " + _RANGE),
    ("ssim_loss_backward", (_P, _P, (1 << 24) + 1, 1, 16, 16, 0, None, _P, _P), 3, "ssim_loss backward: " + _RANGE),
    ("ssim_loss_backward", (_P, _P, 1 << 24, 1, 33, 16, 0, None, _P, _P), 3, "ssim_loss backward: " + _RANGE),
    ("ssim_loss_forward", (_P, _P, 1, 1, 16, 16, 0, _P, _P + 4), 3, "ssim_loss forward: the workspace must be 8-byte aligned"),
    ("ssim_loss_backward", (_P, _P, 1, 1, 16, 16, 0, None, _P, _P + 4), 3, "ssim_loss backward: the workspace must be 8-byte aligned"),
    # B C H W == 0: a successful no-op, whatever the pointers
    ("ssim_loss_forward", (None, None, 0, 1, 16, 16, 0, None, None), 0, None),
    ("ssim_loss_forward", (None, None, 1, 0, 16, 16, 0, None, None), 0, None),
    ("ssim_loss_forward", (None, None, 1, 1, 0, 16, 1, None, None), 0, None),
    ("ssim_loss_backward", (None, None, 1, 1, 16, 0, 0, None, None, None), 0, None),
    ("ssim_loss_backward", (None, None, 0, 3, 16, 16, 1, None, None, None), 0, None),
    # the L2 entry: the L1 entry's rules
    ("l2_mean_forward_grad", (_P, _P, 0, _P, _P, _P), 2, "l2: bad size"),
    ("l2_mean_forward_grad", (_P, _P, -4, _P, _P, _P), 2, "l2: bad size"),
    ("l2_mean_forward_grad", (_P, _P, (1 << 40) + 1, _P, _P, _P), 2, "l2: bad size"),
    ("l2_mean_forward_grad", (None, _P, 8, _P, _P, _P), 1, "l2: null pointer"),
    ("l2_mean_forward_grad", (_P, None, 8, _P, _P, _P), 1, "l2: null pointer"),
    ("l2_mean_forward_grad", (_P, _P, 8, None, _P, _P), 1, "l2: null pointer"),
    ("l2_mean_forward_grad", (_P, _P, 8, _P, None, _P), 1, "l2: null pointer"),
    ("l2_mean_forward_grad", (_P, _P, 8, _P, _P, None), 1, "l2: null pointer"),
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
    rc = getattr(lib, "sstem_%s_f32" % name)(*args, None)
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


def test_python_layer_refusals():
    from loss.loss_ssim import SSIMLoss, ssim
    import train_utils
    x = torch.zeros(1, 1, 16, 16)
    with pytest.raises(NotImplementedError):
        SSIMLoss(window_size=7)
    with pytest.raises(NotImplementedError):
        ssim(x, x, window_size=5)
    with pytest.raises(NotImplementedError):
        SSIMLoss()(x, x)
    with pytest.raises(NotImplementedError):
        ssim(x, x)
    with pytest.raises(NotImplementedError):
        train_utils.SSIMMeanLoss("cpu")(x, x)
    with pytest.raises(NotImplementedError):
        train_utils.L2MeanLoss("cpu")(x, x)
    # the dtype check needs device tensors to be reached; on the meta-free CPU path it is the helper that is asked
    from loss.loss_ssim import _check_ssim_loss_images

    class _OnDevice:
        """A stand-in with a device tensor's answers (no device here)."""
        is_cuda = True

        def __init__(self, dtype, shape):
            self.dtype, self.shape = dtype, torch.Size(shape)

        def dim(self):
            return len(self.shape)
    with pytest.raises(TypeError):
        _check_ssim_loss_images(_OnDevice(torch.float16, (1, 1, 8, 8)), _OnDevice(torch.float16, (1, 1, 8, 8)))
    with pytest.raises(TypeError):
        _check_ssim_loss_images(_OnDevice(torch.float32, (1, 1, 8, 8)), _OnDevice(torch.float64, (1, 1, 8, 8)))
    with pytest.raises(ValueError):
        _check_ssim_loss_images(_OnDevice(torch.float32, (1, 1, 8, 8)), _OnDevice(torch.float32, (1, 1, 8, 9)))
    _check_ssim_loss_images(_OnDevice(torch.float32, (2, 3, 5, 7)), _OnDevice(torch.float32, (2, 3, 5, 7)))     # narrower than 11: legal


def test_steps_reject_unknown_loss_names():
    import steps
    for name in ("L2", "perceptual", "mse"):
        with pytest.raises(AttributeError, match="No this loss function!"):
            steps.IFNetStep("cpu", loss=name)                # refused before any module is built or moved to a device
    for name in ("ssim", "L1", "perceptual"):
        with pytest.raises(AttributeError, match="No this loss function!"):
            steps.UnfoldStep("cpu", loss=name)
