"""steps.UnfoldStep and the backward pass through the SFF FusionNet(6, 2, 32) in train mode, against the REFERENCE class's own step on
the CPU (tests/golden/make_unfold_step_golden.py: sff_scripts_unfolding/main_flowfusionnet.py:198-215 with L1).  The pass goes through
the in-place LeakyReLU blocks, the residual add inside conv_2's store, the (deconv + skip) / 2 in the ConvTranspose store and the
2-channel head; tests/golden/steps.npz pins the other nets, not this one.

``_check`` is tests/test_steps_gpu.py's rule with its constants (see that module's docstring for their derivation): the loss within
LOSS_REL, a gradient norm within max(BASE_REL, COND_FACTOR x the step's conditioning) plus a floor of NORM_FLOOR of the largest norm, a
gradient stored in full within max(BASE_REL, COND_FACTOR x its own conditioning) of its largest element."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from model.model_fusionnet import FusionNet as SffFusionNet
from weight_recipe import fill_, input_for

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("conv_algo_matrix")]
SEED = 555
TARGET_PIXELS = 4.0
LOSS_REL, BASE_REL, COND_FACTOR, NORM_FLOOR = 2e-5, 2e-5, 8.0, 1e-5


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "unfold_step.npz")), json.load(open(os.path.join(golden_dir, "unfold_step_names.json")))


def _check(net, loss, tag, gold):
    z, names = gold
    ref_loss = float(z[tag + "_loss"])
    assert abs(loss.item() - ref_loss) <= LOSS_REL * abs(ref_loss), "loss %.8g vs reference %.8g" % (loss.item(), ref_loss)
    params = dict(net.named_parameters())
    assert list(params) == names[tag]["params"]                      # same parameters, same order as the reference class
    worst = (0.0, None, 0.0)
    norms_ref = z[tag + "_grad_norms"]
    floor = NORM_FLOOR * float(norms_ref.max())
    step_cond = float(z[tag + "_norm_cond"][norms_ref > floor].max())      # the step's noise scale
    for n, ref in zip(names[tag]["params"], norms_ref):
        g = params[n].grad
        if ref < 0:
            assert g is None, "%s has a gradient; the reference leaves it None" % n
            continue
        assert g is not None, "%s has no gradient" % n
        assert torch.isfinite(g).all()
        got = float(g.double().norm())
        rel_tol = max(BASE_REL, COND_FACTOR * step_cond) if ref > floor else 0.0
        if ref > floor:
            worst = max(worst, (abs(got - ref) / ref, n, rel_tol))
        assert abs(got - ref) <= rel_tol * ref + floor, \
            "|grad %s| = %.6g vs reference %.6g (rel %.2e, allowed %.2e + floor %.1e)" % (n, got, ref, abs(got - ref) / (ref + 1e-30), rel_tol, floor)
    for k, n in enumerate(names[tag]["full"]):
        ref = z["%s_grad%d" % (tag, k)].astype(np.float64)
        tol = max(BASE_REL, COND_FACTOR * float(z["%s_grad%d_cond" % (tag, k)]))
        got = params[n].grad.detach().cpu().double().numpy()
        err = np.abs(got - ref).max() / np.abs(ref).max()
        assert err <= tol, "grad %s: max err / max|g| = %.3e, allowed %.3e (COND_FACTOR x the reference's own fp32-vs-fp64 %.1e)" % (
            n, err, tol, float(z["%s_grad%d_cond" % (tag, k)]))
    print("%s: loss %.8g (reference %.8g); worst gradient-norm deviation %.2e at %s (allowed %.2e)" % (tag, loss.item(), ref_loss, worst[0], worst[1], worst[2]))
    return worst


def _batch():
    x = input_for(SEED, "unf_in", (2, 6, 64, 64)).cuda()
    target = ((input_for(SEED, "unf_tg", (2, 2, 64, 64)) * 2.0 - 1.0) * TARGET_PIXELS).cuda()
    return x, target


def test_unfold_step_matches_reference(gold):
    z, names = gold
    assert names["unfold"]["full"] == ["down_1.conv_1.0.weight", "out.weight"]
    net = SffFusionNet(6, 2, 32).train(); fill_(net, SEED + 7); net.cuda()
    x, target = _batch()
    loss = F.l1_loss(net(x), target)
    loss.backward()
    _check(net, loss, "unfold", gold)
    rm = net.state_dict()["down_1.conv_1.1.running_mean"].cpu().double().numpy()
    assert np.abs(rm - z["unfold_bn_running_mean"]).max() <= 2e-5 * np.abs(z["unfold_bn_running_mean"]).max() + 1e-7


def test_unfold_step_object_matches_reference(gold):
    """The same step through steps.UnfoldStep (native L1 launch, flat gradient bucket) with the fixture's weights and batch."""
    import steps
    net = SffFusionNet(6, 2, 32); fill_(net, SEED + 7)
    st = steps.UnfoldStep(torch.device("cuda"), global_batch=2, size=64, net=net)
    st.load(*_batch())
    st.forward_backward()
    torch.cuda.synchronize()
    _check(st.net, st.loss, "unfold", gold)


def _new_step(**kw):
    import steps
    return steps.UnfoldStep(torch.device("cuda"), global_batch=2, size=64, **kw)


def test_one_step_changes_every_parameter_that_has_a_gradient():
    import steps
    import train_utils
    st = _new_step()
    assert st.net.training and st.x.shape == (2, 6, 64, 64) and st.target.shape == (2, 2, 64, 64)
    assert st.loss_name == "l1" and isinstance(st.criterion, train_utils.L1MeanLoss)
    assert st.flop_per_step() == 3 * steps.FusionStep.FLOW_FWD_FLOP_PER_SAMPLE * 2 * (64 / 256.0) ** 2
    before = {n: p.detach().clone() for n, p in st.net.named_parameters()}
    st.step()
    torch.cuda.synchronize()
    assert torch.isfinite(st.loss) and float(st.loss) > 0
    for n, p in st.net.named_parameters():
        assert p.grad is not None, n
        if float(p.grad.abs().max()) > 0:
            assert not torch.equal(p.detach(), before[n]), "%s did not move" % n
    for n, p in st.net.named_parameters():
        if p.dim() == 4:                                     # every convolution's weights are live
            assert float(p.grad.abs().max()) > 0, n


def test_graph_follows_the_eager_trajectory_bit_for_bit():
    eager, graphed = _new_step(), _new_step(graph=True)
    assert graphed.graphed, graphed.graph_error
    assert torch.equal(eager.flat.flat, graphed.flat.flat)
    for _ in range(3):
        eager.step(); graphed.step()
        torch.cuda.synchronize()
        assert float(eager.loss) == float(graphed.loss)
        assert torch.equal(eager.buckets[0].flat, graphed.buckets[0].flat)
        assert torch.equal(eager.flat.flat, graphed.flat.flat)
    for (n, a), (_, b) in zip(eager.net.named_buffers(), graphed.net.named_buffers()):
        assert torch.equal(a, b), n


def test_l2_runs():
    import train_utils
    st = _new_step(loss="l2")
    assert st.loss_name == "l2" and isinstance(st.criterion, train_utils.L2MeanLoss)
    before = st.flat.flat.clone()
    st.forward_backward()
    torch.cuda.synchronize()
    assert torch.isfinite(st.loss) and float(st.loss) > 0 and torch.isfinite(st.buckets[0].flat).all()
    st.step()
    torch.cuda.synchronize()
    assert not torch.equal(st.flat.flat, before)


def test_validate_is_the_epe_of_an_eval_forward_and_leaves_the_net_as_it_was():
    from loss.multiscaleloss import EPE
    st = _new_step()
    st.step()
    torch.cuda.synchronize()
    buffers = {n: b.clone() for n, b in st.net.named_buffers()}
    x, gt = _batch()
    got = st.validate(x, gt)
    assert got.dim() == 0 and got.is_cuda and got.dtype == torch.float32
    assert st.net.training
    for n, b in st.net.named_buffers():
        assert torch.equal(b, buffers[n]), n
    st.net.eval()
    with torch.no_grad():
        pred = st.net(x)
    st.net.train()
    assert float(got) == float(EPE(pred, gt))
    # equal-sized images: the mean of the reference's per-image EPEs
    per_image = torch.stack([(pred[i:i + 1] - gt[i:i + 1]).double().pow(2).sum(1).sqrt().mean() for i in range(2)]).mean()
    assert abs(float(got) - float(per_image)) <= 1e-6 * float(per_image)


def test_unknown_loss_names_raise():
    import steps
    for name in ("ssim", "perceptual", "L1"):
        with pytest.raises(AttributeError, match="No this loss function!"):
            steps.UnfoldStep(torch.device("cuda"), global_batch=2, size=64, loss=name)
