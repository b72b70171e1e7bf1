"""The back-warp's gradient contract on the CPU: tests/warp_grad_ref64.py (the float64 restatement the GPU tests hold the kernels to)
against tests/golden/warp_grad.npz -- the REFERENCE module's own fp32 autograd (tests/golden/make_warp_grad_golden.py) -- at every
element, five-plus deliberate mistakes of the restatement that the fixture must each catch, and the new entry's refusals.

Bounds (u = 2^-24; S, k, A per element from ref64):
    flow gradient   (C + 8) u S      image gradient   (k + 4) u A
The reference's autograd path takes, for one flow-gradient element: g*I (1), the channel sum of the broadcast weight's gradient
(C - 1), times the other axis' weight (1), the four taps' terms accumulated into dx (3), and the weights wa..wd's own rounding reaching
the forward only -- C + 4 in all, inside C + 8.  For one image-gradient element: w = wx*wy (1), w*g (1), then the scatter-adds of the
four gathers and the sum of their four buffers, k - 1 adds -- k + 1, inside k + 4."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import sstem_native
import warp_grad_ref64 as R

CASES = ("rand", "knots", "zero", "sides", "p1x1", "c1", "many")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "warp_grad.npz"))


def _case(gold, name):
    return gold[name + "_img"], gold[name + "_flow"], gold[name + "_g"]


def _violations(gold, name, mutant=None):
    """(flow-gradient elements outside their bound, image-gradient elements outside theirs, worst ratios)."""
    img, flow, g = _case(gold, name)
    r = R.ref64(img, flow, g, mutant)
    C = img.shape[1]
    ef = np.abs(gold[name + "_grad_flow"].astype(np.float64) - r["grad_flow"])
    ei = np.abs(gold[name + "_grad_img"].astype(np.float64) - r["grad_image"])
    bf, bi = R.flow_bound(r, C + 8), R.image_bound(r, 4)
    ratio = lambda e, b: float((e / np.maximum(b, 1e-300)).max()) if e.size else 0.0       # noqa: E731
    return int((ef > bf).sum()), int((ei > bi).sum()), ratio(ef, bf), ratio(ei, bi)


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_reference_autograd_at_every_element(gold, name):
    nf, ni, rf, ri = _violations(gold, name)
    print("%s: worst error / bound: flow gradient %.3f, image gradient %.3f" % (name, rf, ri))
    assert nf == 0 and ni == 0
    img, flow, g = _case(gold, name)
    r = R.ref64(img, flow, g)
    assert np.abs(gold[name + "_out"] - r["out"]).max() <= 5 * R.U * max(1.0, float(r["out_abs"].max()))


def test_fixture_covers_what_it_is_meant_to(gold):
    assert gold["rand_img"].shape == (2, 3, 9, 13) and float(np.abs(gold["rand_flow"]).max()) <= 4.0
    assert not gold["zero_flow"].any() and np.array_equal(gold["zero_grad_img"], gold["zero_g"])        # identity warp: dL/dimage = g
    f = gold["knots_flow"]
    assert ((f * 2) == np.round(f * 2)).all() and (f == np.round(f)).any() and (f != np.round(f)).any()
    x0, x1, y0, y1, wx, wy = R.taps(gold["sides_flow"])
    H, W = gold["sides_img"].shape[2:]
    x = (x1.astype(np.float64) - wx)[0, :, 0]                          # the padded coordinate each row of sample 0 lands on
    for v in (0.0, 1.0, float(W), float(W + 1)):
        assert (x == v).any(), v
    assert (x < 0).any() and (x > W + 1).any()
    y = (y1.astype(np.float64) - wy)[1, 0, :]
    for v in (0.0, 1.0, float(H), float(H + 1)):
        assert (y == v).any(), v
    assert (y < 0).any() and (y > H + 1).any()
    assert gold["p1x1_img"].shape[2:] == (1, 1) and gold["c1_img"].shape[1] == 1
    r = R.ref64(*_case(gold, "many"))
    assert gold["many_img"].shape == (1, 2, 5, 7) and int(r["k"].max()) == 35 and int((r["k"] > 0).sum()) == 2 * 4
    # pixels that sample outside the padded plane have zero gradients in the reference too
    out = np.broadcast_to(((x0 == x1) | (y0 == y1))[:, None], gold["sides_grad_flow"].shape)
    assert out.any() and not gold["sides_grad_flow"][out].any()


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_each_mutant_of_the_restatement_fails_the_fixture(gold, mutant):
    caught = [name for name in CASES if sum(_violations(gold, name, mutant)[:2]) > 0]
    print("%s: caught by %s" % (mutant, caught))
    assert caught, "the fixture does not notice the mutant %s" % mutant


# ---- the entry's refusals: no device is visible in the child, so a call that passed validation would end as status 4 --------------
_CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
import sstem_native
lib = sstem_native.load_library()
n = ctypes.c_int(0)
path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
rc = ctypes.CDLL(path).hipGetDeviceCount(ctypes.byref(n))
if rc == 0 and n.value > 0:
    print(json.dumps({"visible": n.value})); sys.exit(0)
def call(fn, *a):
    rc = getattr(lib, fn)(*a)
    return [rc, lib.sstem_last_error().decode() if rc else None]
I, F, G, GF, GI = 4096, 8192, 12288, 16384, 20480         # never dereferenced: every row is refused or empty
bwd = lambda *a: call("sstem_warp_bilinear_backward_f32", *a)
rows = {
  "both_outputs_null": bwd(I, F, G, None, None, 0, 2, 3, 8, 8, None),
  "null_flow": bwd(I, None, G, GF, GI, 0, 2, 3, 8, 8, None),
  "null_grad_output": bwd(I, F, None, GF, GI, 0, 2, 3, 8, 8, None),
  "null_image_with_grad_flow": bwd(None, F, G, GF, None, 0, 2, 3, 8, 8, None),
  "all_null": bwd(None, None, None, None, None, 0, 2, 3, 8, 8, None),
  "negative": bwd(I, F, G, GF, GI, 0, -1, 3, 8, 8, None),
  "negative_and_null": bwd(None, F, G, GF, GI, 0, -1, 3, 8, 8, None),
  "too_large": bwd(I, F, G, GF, GI, 0, 2, 3, 65536, 32768, None),
  "plane_limit_ok_null": bwd(None, None, None, None, None, 0, 2, 3, 65536, 32764, None),
  "too_many": bwd(I, F, G, GF, GI, 1, 1099511627777, 3, 8, 8, None),
  "empty_B": bwd(None, None, None, None, None, 0, 0, 3, 8, 8, None),
  "empty_C": bwd(None, None, None, None, None, 0, 2, 0, 8, 8, None),
  "empty_H": bwd(None, None, None, None, None, 1, 2, 3, 0, 8, None),
  "empty_W": bwd(None, None, None, None, None, 0, 2, 3, 8, 0, None),
}
fwd = lambda *a: call("sstem_warp_bilinear_f32", *a)
twin = {
  "all_null": fwd(None, None, None, 2, 3, 8, 8, None),
  "negative": fwd(I, F, G, -1, 3, 8, 8, None),
  "negative_and_null": fwd(None, F, G, -1, 3, 8, 8, None),
  "too_large": fwd(I, F, G, 2, 3, 65536, 32768, None),
  "plane_limit_ok_null": fwd(None, None, None, 2, 3, 65536, 32764, None),
  "too_many": fwd(I, F, G, 1099511627777, 3, 8, 8, None),
  "empty_B": fwd(None, None, None, 0, 3, 8, 8, None),
  "empty_C": fwd(None, None, None, 2, 0, 8, 8, None),
  "empty_H": fwd(None, None, None, 2, 3, 0, 8, None),
  "empty_W": fwd(None, None, None, 2, 3, 8, 0, None),
}
print(json.dumps({"rows": rows, "twin": twin}))
"""


def test_entry_refusals_without_a_device(repo_root):
    import json
    assert "sstem_warp_bilinear_backward_f32" in sstem_native.C_ABI
    lib = ctypes.CDLL(sstem_native.library_path())
    assert hasattr(lib, "sstem_warp_bilinear_backward_f32")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(repo_root, "sstem-restoration_amd")], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    if "visible" in got:
        pytest.skip("the child process sees a device despite HIP_VISIBLE_DEVICES=-1: nothing called")
    rows, twin = got["rows"], got["twin"]
    null = [1, "warp backward: null tensor pointer"]
    for k in ("both_outputs_null", "null_flow", "null_grad_output", "null_image_with_grad_flow", "all_null", "plane_limit_ok_null"):
        assert rows[k] == null, (k, rows[k])
    for k in ("negative", "negative_and_null", "too_large", "too_many"):
        assert rows[k] == [2, "warp backward: bad shape"], (k, rows[k])
    for k in ("empty_B", "empty_C", "empty_H", "empty_W"):
        assert rows[k] == [0, None], (k, rows[k])
    # the forward's answers for the same numbers: the same status, the same message after the family's prefix
    for k, (status, text) in twin.items():
        assert rows[k][0] == status, (k, rows[k], status)
        assert (rows[k][1] or "").replace("warp backward:", "warp:") == (text or ""), (k, rows[k], text)
