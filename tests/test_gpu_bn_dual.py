"""Dual-BN kernels (a Residual whose skip is conv+BN) against the kernels
they replace, bit for bit: the dual forward against bn_act_fwd twice, the
dual backward against bn_act_bwd twice, and a Residual(64, 128) module
forward+backward against the same module run with RTHD_BN_DUAL=0 in a fresh
process. Run as a script (`python test_gpu_bn_dual.py OUT.pt`) this file is
that process: it writes the module results to OUT.pt.
"""

import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CL = torch.channels_last
B = 2


def _C():
    from real_time_helmet_detection_amd.ops import _backend
    return _backend.require_ext()


def _tensors(hw, c):
    h, w = hw
    g = torch.Generator().manual_seed(100 * h + c)

    def act_t():
        t = torch.randn(B, c, h, w, generator=g).to('cuda', torch.bfloat16)
        return t.contiguous(memory_format=CL)

    def vec(lo, hi):
        return (torch.rand(c, generator=g) * (hi - lo) + lo).cuda()

    t = dict(x=act_t(), xs=act_t(), dy=act_t(),
             gamma=vec(0.5, 1.5), beta=vec(-0.5, 0.5),
             gamma_s=vec(0.5, 1.5), beta_s=vec(-0.5, 0.5))
    t['mean'], t['rstd'] = _C().bn_stats(t['x'], None, None, 0.1, 1e-5)
    t['mean_s'], t['rstd_s'] = _C().bn_stats(t['xs'], None, None, 0.1, 1e-5)
    return t


# (48, 64): more than 8 row chunks on either path, so the sums also pass
# through the sliced stage of the finish
@pytest.mark.parametrize('act', [1, 0], ids=['ReLU', 'Linear'])
@pytest.mark.parametrize('c', [64, 128, 24])     # octet, octet, scalar path
@pytest.mark.parametrize('hw', [(8, 8), (12, 20), (48, 64)])
def test_dual_kernels_equal_composition(hw, c, act):
    _check_dual_kernels(hw, c, act)


@pytest.mark.parametrize('c', [64, 128])
def test_dual_octet_kernels_equal_composition_lrelu(c):
    """LReLU's derivative 0.01 makes dy*act' inexact, so this is the case
    that tells a fused from an unfused accumulate."""
    _check_dual_kernels((12, 20), c, 2)


def _check_dual_kernels(hw, c, act):
    C = _C()
    t = _tensors(hw, c)
    main = (t['mean'], t['rstd'], t['gamma'], t['beta'])
    skip = (t['mean_s'], t['rstd_s'], t['gamma_s'], t['beta_s'])

    s = C.bn_act_fwd(t['xs'], *skip, 0, None)
    want_y = C.bn_act_fwd(t['x'], *main, act, s)
    got_y = C.bn_act_fwd_dual(t['x'], *main, t['xs'], *skip, act)
    assert torch.equal(got_y, want_y)

    dx, dgamma, dbeta, dskip = C.bn_act_bwd(t['dy'], t['x'], *main, act, s)
    dxs, dgamma_s, dbeta_s = C.bn_act_bwd(dskip, t['xs'], *skip, 0, None)
    got = C.bn_act_bwd_dual(t['dy'], t['x'], *main, t['xs'], *skip, act)
    want = (dx, dgamma, dbeta, dxs, dgamma_s, dbeta_s)
    names = ('dpre', 'dgamma', 'dbeta', 'dpre_s', 'dgamma_s', 'dbeta_s')
    for name, a, b in zip(names, got, want):
        assert a.abs().max().item() > 0, name
        assert torch.equal(a, b), name


def _module_results():
    """Residual(64, 128) forward + backward in bf16 training mode: output,
    input gradient, every parameter gradient and the BN buffers."""
    from real_time_helmet_detection_amd import amp
    from real_time_helmet_detection_amd.models.hourglass import Residual
    torch.manual_seed(3)
    net = Residual(64, 128).cuda().to(memory_format=CL).train()
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith('bn.weight'):
                p.uniform_(0.5, 1.5)
            elif name.endswith('bn.bias'):
                p.uniform_(-0.5, 0.5)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 64, 16, 32, generator=g).cuda()
    x = x.contiguous(memory_format=CL).requires_grad_(True)
    dy = torch.randn(2, 128, 16, 32, generator=g).cuda()
    from real_time_helmet_detection_amd.ops import hip
    with amp.autocast(True):
        dual = hip.dual_bn_applies(x, net.conv2.convolution, net.conv2.bn,
                                   'ReLU', x, net.skip.convolution,
                                   net.skip.bn, True)
        y = net(x)
    y.backward(dy.to(y.dtype))
    torch.cuda.synchronize()
    out = {'y': y.detach(), 'dx': x.grad}
    for name, p in net.named_parameters():
        out['grad:' + name] = p.grad
    for name, b in net.named_buffers():
        out['buf:' + name] = b
    out['dual_path'] = torch.tensor(int(dual))
    return {k: v.detach().cpu() for k, v in out.items()}


def _run_module(tmp_path, dual):
    """_module_results in a fresh process. Both processes take the conv
    dispatch heuristic (no first-sight timing), so they run the same conv
    variants and differ in the BN path alone."""
    out = str(tmp_path / ('dual.pt' if dual else 'separate.pt'))
    env = dict(os.environ)
    env['PYTHONPATH'] = REPO
    env['RTHD_NO_AUTOTUNE'] = '1'
    env.pop('RTHD_BN_DUAL', None)
    if not dual:
        env['RTHD_BN_DUAL'] = '0'
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out],
                       cwd=REPO, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    return torch.load(out)


def test_residual_module_equals_separate_path(tmp_path):
    got = _run_module(tmp_path, True)
    want = _run_module(tmp_path, False)
    assert got.pop('dual_path') == 1 and want.pop('dual_path') == 0
    assert set(got) == set(want)
    assert any(k.startswith('grad:skip.') for k in got)
    for k in sorted(got):
        assert got[k] is not None and torch.equal(got[k], want[k]), k


if __name__ == '__main__':
    sys.path.insert(0, REPO)
    torch.save(_module_results(), sys.argv[1])
