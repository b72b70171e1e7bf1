"""Generates tests/golden/unfold_step.npz and unfold_step_names.json: ONE training step of the reference's unfolding-flow predictor
(sff_scripts_unfolding/main_flowfusionnet.py:198-215 with cfg.TRAIN.loss = 'L1', PAD = 0, no weight decay) on the CPU, written as
tests/golden/make_step_goldens.py writes a step (its ``record``: the step in fp32 and in float64, the per-quantity deviations stored as
the conditioning the GPU test derives its tolerances from).

  unfold : sff_scripts_unfolding/model/model_fusionnet.py FusionNet(6, 2, 32).train() -> L1 against the flow label -> backward, through
           the in-place LeakyReLU blocks, the residual add of conv_2, the (deconv + skip) / 2 merges and the 2-channel head.

Weights: fill_(net, SEED + 7) (the flow net's seed in make_step_goldens.py).  Input: input_for(SEED, "unf_in", (2,6,64,64)); target:
input_for(SEED, "unf_tg", (2,2,64,64)) mapped to [-TARGET_PIXELS, TARGET_PIXELS]: a flow label of a few pixels.  The generator checks that the
step's conditioning (the largest fp32-vs-float64 deviation of a live parameter's gradient norm) is of the size steps.npz shows for
the other BatchNorm nets, 1.4e-3 .. 2.2e-3: a far larger one would be answered by the input scale, not by a tolerance.  Measured
5.0e-3 at +-4 px, the smallest of the label scales 1, 2, 3, 4, 6, 8 px (5.0e-3 .. 1.2e-2: this net is some fifty layers deep, twice the
U-Nets' depth) -- the same order, so the scale stays at 4.

Stored: loss, loss64, grad_norms, norm_cond, two gradients in full (down_1.conv_1.0.weight, out.weight) with their _cond, and one
BatchNorm running mean after the step's forward.

Run from the repo root:  python tests/golden/make_unfold_step_golden.py
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_model_goldens as G  # noqa: E402  (stubs + loader of the reference files; also puts tests/ on the path)
import make_step_goldens as S  # noqa: E402
from weight_recipe import fill_, input_for  # noqa: E402

SEED = 555
TARGET_PIXELS = 4.0
FULL = ["down_1.conv_1.0.weight", "out.weight"]
RUNNING_MEAN = "down_1.conv_1.1.running_mean"
COND_RANGE = (1.4e-3, 2.2e-3)          # steps.npz: the BatchNorm nets' step conditioning


def inputs():
    x = input_for(SEED, "unf_in", (2, 6, 64, 64))
    target = (input_for(SEED, "unf_tg", (2, 2, 64, 64)) * 2.0 - 1.0) * TARGET_PIXELS
    return x, target


def generate():
    torch.set_num_threads(8)
    G.install_stubs()
    mf = G.load_ref("sff_scripts_unfolding/model/model_fusionnet.py", "ref_unfold_model_fusionnet")
    x, target = inputs()
    out, names = {}, {}

    def build():
        n = mf.FusionNet(input_nc=6, output_nc=2, ngf=32).train(); fill_(n, SEED + 7); return n
    net = S.record(out, names, "unfold", build, lambda n, dt: F.l1_loss(n(x.to(dt)), target.to(dt)), FULL)
    out["unfold_bn_running_mean"] = net.state_dict()[RUNNING_MEAN].numpy().copy()
    return out, names


def step_conditioning(out):
    norms = out["unfold_grad_norms"]
    return float(out["unfold_norm_cond"][norms > 1e-5 * norms.max()].max())


if __name__ == "__main__":
    out, names = generate()
    cond = step_conditioning(out)
    print("step conditioning %.3e (the other BatchNorm nets: %.1e .. %.1e)" % (cond, COND_RANGE[0], COND_RANGE[1]))
    assert cond <= 3 * COND_RANGE[1], "ill-conditioned step: change the input scale, not the tolerance"
    np.savez_compressed(os.path.join(HERE, "unfold_step.npz"), **out)
    with open(os.path.join(HERE, "unfold_step_names.json"), "w") as f:
        json.dump(names, f, indent=0)
    for k, v in out.items():
        v = np.asarray(v)
        print("%-30s %-16s absmax %.5g" % (k, v.shape, np.abs(v).max()))
    print("unfold_step.npz", os.path.getsize(os.path.join(HERE, "unfold_step.npz")), "bytes")
