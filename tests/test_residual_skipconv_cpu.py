"""functional.conv_bn_act_skipconv on CPU tensors is the two conv_bn_act
calls it stands for: a Residual whose skip is conv+BN computes what it did
when its forward spelled the two calls out."""

import copy

import torch

from real_time_helmet_detection_amd.models.hourglass import Residual
from real_time_helmet_detection_amd.ops import functional as F2


def _spelled_out(net, x):
    y1 = net.conv1(x)
    s = net.skip(x)
    return net.conv2(y1, skip=s, act_override=net.activation.name)


def test_residual_skipconv_matches_two_calls():
    torch.manual_seed(0)
    a = Residual(8, 16).train()
    b = copy.deepcopy(a)
    x = torch.randn(2, 8, 6, 10)
    xa = x.clone().requires_grad_(True)
    xb = x.clone().requires_grad_(True)
    ya = a(xa)
    yb = _spelled_out(b, xb)
    assert torch.equal(ya, yb)
    ya.square().sum().backward()
    yb.square().sum().backward()
    assert torch.equal(xa.grad, xb.grad)
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(p.grad, q.grad), n
    for (n, p), (_, q) in zip(a.named_buffers(), b.named_buffers()):
        assert torch.equal(p, q), n


def test_skipconv_eval_matches_two_calls():
    torch.manual_seed(1)
    net = Residual(8, 16).eval()
    x = torch.randn(1, 8, 4, 4)
    with torch.no_grad():
        got = F2.conv_bn_act_skipconv(
            net.conv1(x), net.conv2.convolution, net.conv2.bn, 'ReLU',
            False, x, net.skip.convolution, net.skip.bn)
        want = _spelled_out(net, x)
    assert torch.equal(got, want)
