"""The native validation scores on the GPU (csrc/score_kernels.hip, include/sstem_score.h, utils/psnr_ssim.py, loss/multiscaleloss.py,
steps.FusionStep.validate / IFNetStep.validate) against ``ref64`` (tests/scores_ref64.py: the reference's formulation in float64).

Bounds:
* SSIM 1e-9 absolute: each blurred moment is a convex combination of at most 143 float64 terms of size <= 65025, so another summation
  order (separable taps against the 2-D window) moves it by <= 143 * 2^-53 * 65025 = 1e-9; the map's denominators are at least C1 C2
  with C2 = 58.5, so a map value, and the mean of the map, moves by <= 3e-10; the bound is three times that.
* mse 1e-12 relative: a sum of non-negative float64 terms, any order is within n * 2^-53 <= 4e-13 for the 4000 pixels here.
* PSNR: recomputed from the native mse with ``math``, 1e-9 dB (device log10 / sqrt against the host's).
* EPE 1e-12 relative against ref64 (float64 result of the launch), and the float32 result of ``EPE`` within 4 D of the reference's own
  output, D = the largest relative deviation of the reference's float32 run from ref64 over the fixture's flow cases (the factor
  tests/test_ms_ssim_gpu.py uses, for the same reason: another summation order is a rounding pattern of the reference's own size).
"""
import math
import os

import numpy as np
import pytest
import torch

import scores_ref64 as R

pytestmark = pytest.mark.gpu

SSIM_TOL, MSE_RTOL, PSNR_TOL, EPE_RTOL = 1e-9, 1e-12, 1e-9, 1e-12


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "scores.npz"))


_refs = {}


def _pair(golden, name):
    return torch.from_numpy(golden[name + "_a"]), torch.from_numpy(golden[name + "_b"])


def _ref(golden, name, swap=False, twice=False):
    """ref64 (mse, psnr, ssim) of a fixture case, or of its exchanged / doubled-first-image variant, computed once on the host."""
    key = (name, swap, twice)
    if key not in _refs:
        a, b = _pair(golden, name)
        a, b = (b, a) if swap else (a, b)
        b = a if twice else b
        _refs[key] = R.score64(a[None], b[None])[0].tolist()
    return _refs[key]


def _check_row(got, want, what):
    mse, psnr, ssim = got
    print("%s: native mse %.17g psnr %.12f ssim %.15f | ref64 mse %.17g psnr %.12f ssim %.15f" % ((what, mse, psnr, ssim) + tuple(want)))
    assert abs(ssim - want[2]) <= SSIM_TOL, what
    assert abs(mse - want[0]) <= MSE_RTOL * want[0], what
    if mse < 1.0e-10:
        assert psnr == 1.0e12 and want[1] == 1.0e12, what
    else:
        assert abs(psnr - 20 * math.log10(1 / math.sqrt(mse))) <= PSNR_TOL, what


@pytest.mark.parametrize("name", list(R.IMAGE_CASES))
def test_fixture_cases_against_ref64(golden, name):
    from utils.psnr_ssim import score_batch
    a, b = _pair(golden, name)
    got = score_batch(a[None].cuda(), b[None].cuda())
    assert got.shape == (1, 3) and got.dtype == torch.float64 and got.is_cuda
    _check_row(got[0].tolist(), _ref(golden, name), name)
    assert abs(float(got[0, 2]) - float(golden[name + "_ssim"])) <= SSIM_TOL          # the reference's own float64 result
    if name == "same":
        assert got[0].tolist() == [0.0, 1.0e12, 1.0]


# B = 3: (case, exchanged?, first image twice?) per image; the 43 x 44 float stack takes a different range branch in every image
_STACKS = {
    "f43x44": [("f43x44", False, False), ("over1", False, False), ("same", False, False)],
    "f75x53": [("f75x53", False, False), ("f75x53", True, False), ("f75x53", False, True)],
    "u43x44": [("u43x44", False, False), ("bits", False, False), ("u43x44", True, False)],
    "u75x53": [("u75x53", False, False), ("u75x53", True, False), ("u75x53", False, True)],
}


@pytest.mark.parametrize("stack", list(_STACKS))
def test_stacks_score_every_image_on_its_own(golden, stack):
    from utils.psnr_ssim import score_batch
    As, Bs = [], []
    for name, swap, twice in _STACKS[stack]:
        a, b = _pair(golden, name)
        a, b = (b, a) if swap else (a, b)
        As.append(a); Bs.append(a if twice else b)
    A, Bt = torch.stack(As).cuda(), torch.stack(Bs).cuda()
    got = score_batch(A, Bt)
    assert got.shape == (3, 3)
    for i, (name, swap, twice) in enumerate(_STACKS[stack]):
        _check_row(got[i].tolist(), _ref(golden, name, swap, twice), "%s[%d]" % (stack, i))
        alone = score_batch(A[i:i + 1], Bt[i:i + 1])
        assert torch.equal(alone[0], got[i]), (stack, i)                 # independent of its neighbours, bit for bit
    assert torch.equal(score_batch(A[:, None], Bt[:, None]), got)        # [B,1,H,W] is the same call


@pytest.mark.parametrize("name", ["f43x44", "f75x53"])
def test_quantisation_is_numpys(golden, name):
    """The f32 entry on x and the u8 entry on (x * 255) truncated to bytes: the same SSIM bits, and the reference's SSIM."""
    from utils.psnr_ssim import score_batch
    a, b = (t[None].cuda() for t in _pair(golden, name))
    f = score_batch(a, b)
    u = score_batch((a * 255).to(torch.uint8), (b * 255).to(torch.uint8))
    assert torch.equal(f[:, 2], u[:, 2])
    for got in (f, u):
        assert abs(float(got[0, 2]) - float(golden[name + "_ssim"])) <= SSIM_TOL


def test_clamp01_determinism_and_negative_values(golden):
    from utils.psnr_ssim import score_batch
    a0, b0 = _pair(golden, "f43x44")
    a1, b1 = _pair(golden, "over1")
    pred = torch.stack((a0 * 1.4 - 0.2, a1 * 1.2 - 0.1)).cuda()          # values below 0 and above 1 in both images
    gt = torch.stack((b0, b1)).cuda()
    assert float(pred.min()) < 0 and float(pred.max()) > 1
    got = score_batch(pred, gt, clamp01=True)
    assert torch.equal(got, score_batch(pred.clamp(0, 1), gt))
    assert torch.equal(got, score_batch(pred, gt, clamp01=True))          # the same bits run to run
    want = R.score64(pred.cpu(), gt.cpu(), clamp01=True)
    for i in range(2):
        _check_row(got[i].tolist(), want[i].tolist(), "clamped[%d]" % i)
    # unclamped, both predictions have a maximum above 1: the `> 1` branch, values as they are
    raw = score_batch(pred, gt)
    want = R.score64(pred.cpu(), gt.cpu())
    for i in range(2):
        _check_row(raw[i].tolist(), want[i].tolist(), "raw[%d]" % i)
    # the documented deviation: a negative value in a unit-range image quantises to 0
    neg = (a0 - 0.25)[None].cuda()
    assert float(neg.max()) <= 1 and float(neg.min()) < 0
    _check_row(score_batch(neg, b0[None].cuda())[0].tolist(), R.score64(neg.cpu(), b0[None])[0].tolist(), "negative")


def test_graph_capture_replays_to_the_same_bits(golden):
    from utils.psnr_ssim import score_batch
    a, b = (torch.stack((t, t.flip(0))).cuda() for t in _pair(golden, "f75x53"))
    eager = score_batch(a, b, clamp01=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        score_batch(a, b, clamp01=True)                  # this stream's workspace exists before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = score_batch(a, b, clamp01=True)
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_compute_psnr_and_compute_ssim_return_what_the_reference_returns(golden):
    from utils.psnr_ssim import compute_psnr, compute_ssim
    a, b = (t.cuda() for t in _pair(golden, "f43x44"))
    got = compute_psnr(a, b)
    assert isinstance(got, tuple) and len(got) == 2 and all(type(v) is float for v in got)
    want = _ref(golden, "f43x44")
    assert abs(got[0] - want[0]) <= MSE_RTOL * want[0] and abs(got[1] - want[1]) <= PSNR_TOL
    assert compute_psnr(a[None, None], b[None]) == got                   # leading singleton dimensions
    s = compute_ssim(a, b)
    assert type(s) is float and abs(s - float(golden["f43x44_ssim"])) <= SSIM_TOL
    same = compute_psnr(a, a)
    assert same == 1000000000000 and type(same) is int
    assert compute_ssim(a, a) == 1.0
    u, v = (t.cuda() for t in _pair(golden, "u75x53"))
    assert abs(compute_ssim(u, v) - float(golden["u75x53_ssim"])) <= SSIM_TOL
    with pytest.raises(ValueError):
        compute_ssim(torch.stack((a, a)), torch.stack((b, b)))
    with pytest.raises(RuntimeError, match="at least 11"):
        compute_ssim(a[:10], b[:10])


@pytest.mark.parametrize("name", list(R.FLOW_CASES))
def test_flow_epe_against_ref64_and_the_reference(golden, name):
    from loss import multiscaleloss as M
    bound = 4.0 * max(float(golden[n + "_dev_epe"].max()) for n in R.FLOW_CASES)
    f, t = torch.from_numpy(golden[name + "_flow"]), torch.from_numpy(golden[name + "_target"])
    fg, tg = f.cuda(), t.cuda()
    for sparse in (False, True):
        for mean in (False, True):
            want = R.epe64(f, t, sparse, mean)
            ref = float(golden[name + "_epe"][int(sparse), int(mean)])
            d = M._epe_float64(fg, tg, sparse, mean)
            v = M.EPE(fg, tg, sparse=sparse, mean=mean)
            assert d.dtype == torch.float64 and v.dtype == torch.float32 and v.dim() == 0 and v.is_cuda
            print("%s sparse %d mean %d: native %.17g ref64 %.17g reference %.9g (bound %.2e)" % (name, sparse, mean, float(d), want, ref, bound))
            if math.isnan(want):
                assert math.isnan(float(d)) and math.isnan(float(v)) and math.isnan(ref)
                continue
            assert abs(float(d) - want) <= EPE_RTOL * abs(want)
            assert abs(float(v) - ref) <= bound * abs(ref)
            assert float(M._epe_float64(fg, tg, sparse, mean)) == float(d)            # the same bits run to run
        assert torch.equal(M.realEPE(fg, tg, sparse=sparse).view(torch.int32), M.EPE(fg, tg, sparse=sparse, mean=True).view(torch.int32))   # (NaN too)
    with pytest.raises(ValueError):
        M.EPE(fg[:, :1], tg[:, :1])
    with pytest.raises(NotImplementedError, match="up-sampling"):
        M.realEPE(fg[:, :, ::2, ::2], tg)


STEP_SIZE = 32


def _buffers(net):
    return {k: v.clone() for k, v in net.named_buffers()}


def _validate_leaves_no_trace(make, by_hand, has_batchnorm):
    """make(): a step object; by_hand(st, x): the eval forward written out.  validate() equals score_batch on that forward, and the
    training state and the next step are what they are on a twin that never validated."""
    from utils.psnr_ssim import score_batch
    st, twin = make(), make()
    st.step(); twin.step()
    torch.cuda.synchronize()
    assert float(st.loss) == float(twin.loss)
    g = torch.Generator(device="cuda"); g.manual_seed(77)
    x = torch.rand(st.batch, 6, STEP_SIZE, STEP_SIZE, device="cuda", generator=g)
    gt = torch.rand(st.batch, 1, STEP_SIZE, STEP_SIZE, device="cuda", generator=g)
    before = _buffers(st.net)
    assert any(k.endswith("running_mean") for k in before) == has_batchnorm          # (the interpolation net has no BatchNorm)
    bucket, batch = st.buckets[0].flat.clone(), [t.clone() for t in (st.x, st.target) + ((st.inp,) if hasattr(st, "inp") else ())]
    psnr = st.validate(x, gt)
    assert psnr.shape == (st.batch,) and psnr.dtype == torch.float64 and psnr.is_cuda and bool(torch.isfinite(psnr).all())
    assert st.net.training
    after = _buffers(st.net)
    assert all(torch.equal(before[k], after[k]) for k in before)
    assert torch.equal(bucket, st.buckets[0].flat)
    assert all(torch.equal(a, b) for a, b in zip(batch, (st.x, st.target) + ((st.inp,) if hasattr(st, "inp") else ())))
    st.net.eval()
    with torch.no_grad():
        pred = by_hand(st, x)
    st.net.train()
    assert torch.equal(psnr, score_batch(pred, gt, clamp01=True)[:, 1])
    want = R.score64(pred[:, 0].cpu(), gt[:, 0].cpu(), clamp01=True)[:, 1]
    assert float((psnr.cpu() - want).abs().max()) <= PSNR_TOL          # (1e-12 of the mse is 4e-12 dB)
    st.step(); twin.step()
    torch.cuda.synchronize()
    assert float(st.loss) == float(twin.loss)
    assert torch.equal(st.flat.flat, twin.flat.flat)


def test_fusion_step_validate():
    import steps

    def by_hand(st, x):
        inp = x.clone()
        inp[:, :3] = st.warp(x[:, :3].contiguous(), st.flow(x).permute(0, 2, 3, 1))
        return st.net(inp)
    _validate_leaves_no_trace(lambda: steps.FusionStep(torch.device("cuda"), global_batch=2, size=STEP_SIZE), by_hand, True)


def test_ifnet_step_validate():
    import steps
    _validate_leaves_no_trace(lambda: steps.IFNetStep(torch.device("cuda"), global_batch=2, size=STEP_SIZE), lambda st, x: st.net(x),
                              False)
