"""The amax invariant at every consumer, on the networks and steps as they run (tests/amax_audit.py): whenever hipnn hands out a word
for a tensor, max|t| <= bound(word) (1 + slack), slack 0 but for words handed through bilinear up-sampling (N_UP_AMAX 2^-24).

Every network of tests/test_models_gpu.py / tests/test_steps_gpu.py (their weight recipe, their 64 x 64 inputs) runs forward without a
gradient and forward + backward, and every training step runs its forward_backward, under HF.ALGO_MFMA_F16X3 and under ALGO_AUTO, on the
recipe's input and on an adversarial one (one pixel per image at 64 times the input's maximum, in a corner: a maximum that sits where
no interior tile sees it and that dwarfs every bound measured on the rest).  Each case also demands a word from every rule its
network's code reaches, so a rule that silently stops tagging cannot pass as clean.  The largest bound-to-maximum ratio is printed."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import amax_audit as AA
import hipnn.functional as HF
import networks
import steps
import stream_ref64 as R
from hipnn import FusedSequential
from model.model_fusionnet import FusionNet as SffFusionNet
from model.model_interp import IFNet as SffIFNet
from model.model_unet import UNet as SffUNet
from test_conv_split_gpu import _close
from weight_recipe import fill_, input_for

pytestmark = pytest.mark.gpu
SEED = 555
ALGOS = {"f16x3": HF.ALGO_MFMA_F16X3, "auto": HF.ALGO_AUTO}


@pytest.fixture(autouse=True)
def _reset_algo():
    yield
    HF.set_algorithm(HF.ALGO_AUTO)


def _adversarial(x):
    """The input with one pixel per image set to 64 times its maximum, at a corner."""
    x = x.clone()
    big = 64.0 * float(x.abs().max())
    for n in range(x.shape[0]):
        x[n, 0, (0, -1)[n % 2], (-1, 0)[n % 2]] = big if n % 2 == 0 else -big
    return x


# (constructor, recipe seed, input names and shapes): tests/test_steps_gpu.py
NETS = {
    "sff_ifnet": (lambda: SffIFNet(51), SEED, [("ifstep_in", (1, 6, 64, 64))]),
    "sff_unet": (lambda: SffUNet(6, 1), SEED + 6, [("step_in", (2, 6, 64, 64))]),
    "sff_fusionnet": (lambda: SffFusionNet(6, 2, 32), SEED + 7, [("step_in", (2, 6, 64, 64))]),
    "sp_unet": (lambda: networks.UNet(1, 1), SEED + 2, [("spu_in", (2, 1, 64, 64))]),
    "sp_fusionnet": (lambda: networks.FusionNet(1, 1), SEED + 3, [("spf_a", (2, 1, 64, 64)), ("spf_b", (2, 1, 64, 64))]),
}

# The rules whose words each network's code ASKS FOR (a consumer calls amax_word_of or measured_amax_word on a tensor the rule tagged),
# per algorithm setting and mode, at these 64 x 64 sizes -- read from model/*.py, networks.py and hipnn/fused.py, and what the audit's
# report shows.  A word from each of them must have been asked for.  "produced:" matches every launch's own bound by prefix.
#   measured              the network input (and whatever reaches a consumer untagged)
#   hand_on:pool_module   the 2 x 2 poolings between the blocks;  hand_on:backward: the average pooling's gradient (IFNet)
#   hand_on:upsample      nn.Upsample inside a FusedSequential (IFNet; networks.Up when a gradient is recorded)
#   concat_upsample       networks.Up without a gradient: the up-sampled half stored straight into the concatenation
#   concat                model_unet's (in-place) concatenations, networks.Up's torch.cat when a gradient is recorded
#   sum                   a residual added outside the launch (FusionNet's conv_1 + conv_3 and skip averages, the IFNet's additive skips)
#   x16                   the up-sampling backward;  hand_on:_check: the copy of a channel slice of a concatenation's gradient
#   hand_on:_alias_of_out the alias autograd returns for out= (model_unet's producers storing into the concatenated tensors)
# Under ALGO_AUTO no inference launch of these sizes takes the fp16 id in the SFF nets (nothing is asked for) and the IFNet's recorded
# launches only measure; the training launches of the other nets carry words as under the forced id.
_P = {"measured", "produced:"}
RULES = {
    ("sff_ifnet", "inference"): _P | {"hand_on:pool_module", "hand_on:upsample", "sum"},
    ("sff_ifnet", "training"): _P | {"hand_on:pool_module", "hand_on:upsample", "sum", "x16", "hand_on:backward"},
    ("sff_unet", "inference"): _P | {"concat", "hand_on:_alias_of_out"},
    ("sff_unet", "training"): _P | {"concat", "hand_on:pool_module"},
    ("sff_fusionnet", "inference"): _P | {"hand_on:pool_module", "sum"},
    ("sff_fusionnet", "training"): _P | {"hand_on:pool_module", "sum"},
    ("sp_unet", "inference"): _P | {"concat_upsample", "hand_on:pool_module"},
    ("sp_unet", "training"): _P | {"concat", "hand_on:_check", "hand_on:pool_module", "hand_on:upsample"},
    ("sp_fusionnet", "inference"): _P | {"concat_upsample", "hand_on:pool_module"},
    ("sp_fusionnet", "training"): _P | {"concat", "hand_on:_check", "hand_on:pool_module", "hand_on:upsample"},
}
RULES_AUTO = {
    ("sff_ifnet", "inference"): set(),
    ("sff_ifnet", "training"): {"measured"},
    ("sff_unet", "inference"): {"measured"},
    ("sff_unet", "training"): _P | {"concat", "hand_on:pool_module"},
    ("sff_fusionnet", "inference"): set(),
    ("sff_fusionnet", "training"): _P | {"hand_on:pool_module", "sum"},
    ("sp_unet", "inference"): _P,
    ("sp_unet", "training"): _P | {"concat", "hand_on:_check", "hand_on:pool_module", "hand_on:upsample"},
    ("sp_fusionnet", "inference"): _P,
    ("sp_fusionnet", "training"): _P | {"concat", "hand_on:_check", "hand_on:pool_module", "hand_on:upsample"},
}
STEPS_AUTO = {"fusion": _P | {"concat", "hand_on:pool_module"}, "ifnet": {"measured"}, "unfold": _P | {"hand_on:pool_module", "sum"}}


def _missing(want, seen):
    return sorted(r for r in want if not any(s == r or (r.endswith(":") and s.startswith(r)) for s in seen))


@pytest.mark.parametrize("algo", sorted(ALGOS))
@pytest.mark.parametrize("name", sorted(NETS))
def test_networks_under_the_audit(name, algo, monkeypatch):
    make, seed, inputs = NETS[name]
    net = make()
    fill_(net, seed)
    net.cuda()
    xs = [input_for(SEED, n, s).cuda() for n, s in inputs]
    HF.set_algorithm(ALGOS[algo])
    silent = []
    for which in ("recipe", "adversarial"):
        ins = xs if which == "recipe" else [_adversarial(x) for x in xs]
        for mode in ("inference", "training"):
            net.train(mode == "training")
            with AA.audit(monkeypatch) as a:
                if mode == "inference":
                    with torch.no_grad():
                        out = net(*[x.clone() for x in ins])
                else:
                    for p in net.parameters():
                        p.grad = None
                    out = net(*[x.clone() for x in ins])
                    F.l1_loss(out, torch.zeros_like(out)).backward()
            tag = "%s %s %s %s" % (name, algo, which, mode)
            print("%s: %s" % (tag, a.report()))
            a.assert_clean()
            assert bool(torch.isfinite(out).all()), tag
            if mode == "training":
                assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in net.parameters()), tag
            want = RULES[(name, mode)] if algo == "f16x3" else RULES_AUTO[(name, mode)]
            if _missing(want, a.rules):
                silent.append("%s: no word from %s; seen %s" % (tag, _missing(want, a.rules), sorted(a.rules)))
    assert not silent, "\n".join(silent)


STEPS = {
    "fusion": (lambda: steps.FusionStep(torch.device("cuda"), global_batch=2, size=64), _P | {"concat", "hand_on:pool_module", "sum"}),
    "ifnet": (lambda: steps.IFNetStep(torch.device("cuda"), global_batch=1, size=64), _P | {"hand_on:pool_module", "hand_on:upsample", "sum", "x16", "hand_on:backward"}),
    "unfold": (lambda: steps.UnfoldStep(torch.device("cuda"), global_batch=2, size=64), _P | {"hand_on:pool_module", "sum"}),
}


@pytest.mark.parametrize("algo", sorted(ALGOS))
@pytest.mark.parametrize("name", sorted(STEPS))
def test_training_steps_under_the_audit(name, algo, monkeypatch):
    HF.set_algorithm(ALGOS[algo])
    make, want = STEPS[name]
    st = make()
    assert not st.graphed
    x0 = st.x.clone()
    silent = []
    want = want if algo == "f16x3" else STEPS_AUTO[name]
    for which in ("recipe", "adversarial"):
        if which == "adversarial":
            st.x.copy_(_adversarial(x0))
            if name == "fusion":                                  # (channels 0 - 2 reach the trained net warped: its own pixel sits in channel 5)
                st.x[:, 5:6] = _adversarial(x0[:, 5:6])
                st.x3.copy_(st.x[:, :3]); st.inp[:, 3:] = st.x[:, 3:]
        with AA.audit(monkeypatch) as a:
            st.forward_backward()
        tag = "%s step %s %s" % (name, algo, which)
        print("%s: %s" % (tag, a.report()))
        a.assert_clean()
        assert bool(torch.isfinite(st.loss).all()) and bool(torch.isfinite(st.buckets[0].flat).all()), tag
        if _missing(want, a.rules):
            silent.append("%s: no word from %s; seen %s" % (tag, _missing(want, a.rules), sorted(a.rules)))
    assert not silent, "\n".join(silent)


# ---- unit cases ----------------------------------------------------------------------------------------------------------------------------
def test_measured_word_of_a_view_bounds_the_view_or_is_refused():
    """measured_amax_word reads x.numel() floats from x.data_ptr(): of a channel slice those are not the slice's elements."""
    base = torch.rand(2, 8, 4, 4, device="cuda")
    base[1, 7, 3, 3] = 50.0                                       # inside the slice, outside the first numel floats behind its pointer
    base[0, 0, 0, 0] = -70.0                                      # outside the slice
    for view in (base[:, 4:], base.transpose(2, 3), base[:, :, ::2], base[1:]):
        try:
            w = HF.measured_amax_word(view)
        except ValueError:
            assert not view.is_contiguous()
            continue
        assert float(w.max()) >= float(view.abs().max()), "a word of %r for a view whose maximum is %r" % (float(w.max()), float(view.abs().max()))
    assert float(HF.measured_amax_word(base[1:]).max()) == 50.0  # a contiguous view is measured, exactly


def test_a_tensor_edited_in_place_between_producer_and_consumer(monkeypatch):
    HF.set_algorithm(HF.ALGO_MFMA_F16X3)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(1, 32, 16, 32, generator=g).cuda()
    w1 = (torch.randn(32, 32, 3, 3, generator=g) * 0.1).cuda(); w2 = (torch.randn(32, 32, 3, 3, generator=g) * 0.1).cuda()
    with torch.no_grad(), AA.audit(monkeypatch) as a:
        mid = HF.conv2d_fused(x, w1)
        assert HF.amax_word_of(mid) is not None
        mid.mul_(4096.0)                                          # 12 binades above the producer's bound: fp16 inf if the stale word were used
        assert HF.amax_word_of(mid) is None
        mid[0, 0, 0, 0] = 3.0e6
        out = HF.conv2d_fused(mid, w2)
    a.assert_clean()
    assert a.rules.get("measured", 0) >= 2, a.rules              # x and the edited tensor
    _close(out, F.conv2d(mid.double().cpu(), w2.double().cpu(), padding=1))


def test_out_aliases_carry_the_launchs_word(monkeypatch):
    HF.set_algorithm(HF.ALGO_MFMA_F16X3)
    g = torch.Generator().manual_seed(10)
    x = torch.randn(2, 32, 16, 32, generator=g).cuda()
    conv = nn.Conv2d(32, 32, 3, padding=1).cuda()
    net = FusedSequential(conv, nn.ReLU())
    with torch.no_grad(), AA.audit(monkeypatch) as a:
        plain = net(x)
        buf = torch.full((2, 32, 16, 32), float("nan"), device="cuda")
        res = net(x, out=buf)
        assert res.data_ptr() == buf.data_ptr() and torch.equal(res, plain)
        cat = torch.full((2, 64, 16, 32), float("nan"), device="cuda")
        blk = net(x, out=cat[:, 32:])
        assert torch.equal(cat[:, 32:], plain)
        for t in (plain, res, buf, blk):
            wd = HF.amax_word_of(t)
            assert wd is not None and float(wd.max()) == float(plain.abs().max())
        assert HF.amax_word_of(cat) is None                      # half of it is not written yet: no bound for the whole
        cat[:, :32] = 1000.0
        assert HF.amax_word_of(blk) is None                      # an edit of the larger tensor: the block's word is stale too
    a.assert_clean()


@pytest.mark.parametrize("scale", [0.5, -0.5, -3.0])
def test_sum_rule_behind_a_recorded_residual(scale, monkeypatch):
    """run_fused's residual outside the launch (a gradient is recorded): (conv(x) + r) * scale tagged by tag_sum_amax."""
    HF.set_algorithm(HF.ALGO_MFMA_F16X3)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 32, 16, 32, generator=g).cuda().requires_grad_()
    net = FusedSequential(nn.Conv2d(32, 32, 3, padding=1), nn.ReLU()).cuda()
    with AA.audit(monkeypatch) as a:
        mid = net(x)
        r = (mid.detach().abs().max() * torch.sign(mid.detach())).clone()          # |r| = the bound everywhere, the sign of the other operand
        HF.measured_amax_word(r)
        y = net(mid, residual=r, res_scale=scale)
        assert HF.amax_word_of(y) is not None
        z = net(y)
    a.assert_clean()
    assert "sum" in a.rules, a.rules
    assert bool(torch.isfinite(z).all())


# ---- bilinear up-sampling on the device: the twin's bits, the excess, the slack -----------------------------------------------------------------
EXCESS_VALUE = 1.0119019746780396      # a float32 whose constant line of 50 pixels comes out one step larger (tests/test_amax_audit_cpu.py)


@pytest.mark.parametrize("shape", [(2, 50, 50), (3, 36, 64), (1, 64, 64), (2, 7, 10)])
def test_upsampling_kernels_compute_the_twin_bit_for_bit_and_exceed_their_input(shape, monkeypatch):
    g = torch.Generator().manual_seed(12)
    x = torch.randn((1,) + shape, generator=g)
    x[0, 0] = EXCESS_VALUE                                        # one constant plane
    got = HF.upsample_bilinear2x(x.cuda())
    twin = torch.from_numpy(R.upsample2x_twin32(x.numpy()))
    assert torch.equal(got.cpu().view(torch.int32), twin.view(torch.int32)), "%d elements differ from the float32 twin" % int((got.cpu() != twin).sum())
    excess = 50 in shape[1:]
    if excess:
        assert float(got[0, 0].max()) > EXCESS_VALUE                  # 'convex: x's bound holds' is not literally true
    assert float(got[0, 0].max()) <= EXCESS_VALUE * (1 + AA.N_UP_AMAX * AA.U)
    m = nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True)
    c = torch.full((1, 2) + shape[1:], EXCESS_VALUE, device="cuda")
    for slack, clean in ((AA.N_UP_AMAX, True), (0, not excess)):
        with torch.no_grad(), AA.audit(monkeypatch, up_slack=slack) as a:
            HF.measured_amax_word(c)
            up = HF.upsample_bilinear2x_module(m, c)
            assert HF.amax_word_of(up) is not None
        assert (not a.violations) == clean, a.report()
        assert "hand_on:upsample" in a.rules
