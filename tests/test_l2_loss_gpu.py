"""The native L2 criterion (include/sstem_io.h: sstem_l2_mean_forward_grad_f32, train_utils.L2MeanLoss) against F.mse_loss + autograd
(cfg.TRAIN.loss = 'L2' of the reference's three SFF loops): the L1 launch's twin, held to the L1 test's bounds."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_utils

pytestmark = pytest.mark.gpu

LOSS_REL = 4e-7         # a fixed-order fp32 sum against the float64 mean: tests/test_edge_and_optim.py's bound for the L1 launch


def _expected_grad(pred, target):
    """fl32(fl32(2 / n) * fl32(pred - target)), evaluated in fp32 on the device."""
    two_inv_n = torch.tensor(np.float32(2.0 / pred.numel()), device=pred.device)
    return two_inv_n * (pred - target)


def _one_step_apart(got, want):
    """Every element within one fp32 step of ``want``."""
    step = torch.maximum(torch.nextafter(want.abs(), torch.full_like(want, float("inf"))) - want.abs(),
                         torch.full_like(want, 1.5e-45))
    return bool(((got - want).abs() <= step).all())


@pytest.mark.parametrize("shape", [(1,), (2,), (3,), (4,), (5,), (2, 1, 33, 31), (2, 2, 64, 64), (3, 1, 257, 255), (4, 1, 512, 600)],
                         ids=lambda s: "x".join(map(str, s)))
def test_loss_and_gradient(shape):
    g = torch.Generator(device="cuda"); g.manual_seed(11 + len(shape) + shape[-1])
    pred = (torch.rand(shape, device="cuda", generator=g) - 0.5) * 6
    target = (torch.rand(shape, device="cuda", generator=g) - 0.5) * 6
    crit = train_utils.L2MeanLoss(pred.device)
    loss, grad = crit(pred, target)
    want64 = float(((pred.double() - target.double()) ** 2).mean())
    rel = abs(float(loss) - want64) / want64
    print("%s: loss %.9g float64 %.9g rel %.2e" % (shape, float(loss), want64, rel))
    assert rel <= LOSS_REL
    assert grad.shape == pred.shape and torch.equal(grad, _expected_grad(pred, target))
    a = pred.clone().requires_grad_(True)
    F.mse_loss(a, target).backward()
    assert _one_step_apart(grad, a.grad)
    # repeated calls on the same (never re-zeroed) workspace: the same bits
    for _ in range(2):
        loss2, grad2 = crit(pred, target)
        assert torch.equal(loss2, loss) and torch.equal(grad2, grad)


def test_unaligned_views_take_the_scalar_path():
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    base_p = torch.rand(4099, device="cuda", generator=g)
    base_t = torch.rand(4099, device="cuda", generator=g)
    crit = train_utils.L2MeanLoss(base_p.device)
    pred, target = base_p[1:], base_t[1:]                    # 4 bytes past a 16-byte boundary
    assert pred.data_ptr() % 16 == 4
    loss, grad = crit(pred, target)
    want64 = float(((pred.double() - target.double()) ** 2).mean())
    assert abs(float(loss) - want64) <= LOSS_REL * want64
    assert torch.equal(grad, _expected_grad(pred, target))
    # the aligned copy of the same numbers: the same gradient bits (the loss may differ by the order of its sum)
    loss_a, grad_a = crit(pred.clone(), target.clone())
    assert torch.equal(grad_a, grad) and abs(float(loss_a) - float(loss)) <= 2 * LOSS_REL * want64


def test_non_finite_values_pass_through():
    pred = torch.tensor([1.0, float("nan"), 2.0, float("inf"), 0.0], device="cuda")
    target = torch.zeros(5, device="cuda")
    loss, grad = train_utils.L2MeanLoss(pred.device)(pred, target)
    assert torch.isnan(loss) and torch.isnan(grad[1]) and torch.isinf(grad[3]) and float(grad[0]) == np.float32(2.0 / 5) and float(grad[4]) == 0.0


def test_graph_capture_replays_equal_eager():
    g = torch.Generator(device="cuda"); g.manual_seed(6)
    pred = torch.rand(2, 1, 64, 64, device="cuda", generator=g); target = torch.rand(2, 1, 64, 64, device="cuda", generator=g)
    crit = train_utils.L2MeanLoss(pred.device)
    l_eager, g_eager = crit(pred, target)
    l_eager, g_eager = l_eager.clone(), g_eager.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        l, gr = crit(pred, target)
    l.zero_(); gr.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(l, l_eager) and torch.equal(gr, g_eager)


def test_backward_from_the_nets_output_gives_autograds_parameter_gradients():
    """``pred.backward(grad)`` with the launch's gradient against ``F.mse_loss(net(x), t).backward()``."""
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        torch.manual_seed(3)
        net = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.Tanh(), torch.nn.Conv2d(8, 2, 3, padding=1)).cuda()
        x = torch.rand(2, 3, 32, 32, device="cuda"); target = torch.rand(2, 2, 32, 32, device="cuda")
        F.mse_loss(net(x), target).backward()
        want = [p.grad.clone() for p in net.parameters()]
        net.zero_grad(set_to_none=True)
        pred = net(x)
        loss, grad = train_utils.L2MeanLoss(x.device)(pred, target)
        pred.backward(grad)
        assert abs(float(loss) - float(F.mse_loss(pred.detach(), target))) <= 2 * LOSS_REL * float(loss)
        for p, w in zip(net.parameters(), want):
            # the two output gradients differ by at most one fp32 step per element: 2e-7 of the parameter gradient's max, summed
            assert float((p.grad - w).abs().max()) <= 1e-6 * float(w.abs().max())
    finally:
        torch.backends.cudnn.deterministic = was
