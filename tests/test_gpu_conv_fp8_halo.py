"""Halo-tile 3x3 fp8 conv (conv_halo_fp8.hip) on the GPU.

The kernel keeps the tap order, the MFMA and the lane -> k map of the
128x128 fp8 kernel, so it must equal conv_fwd_fp8r_tile128 bit for bit; it is
also held to the torch conv on the dequantised values with the bounds of
test_conv_fwd_fp8_resident. The tile is 8 rows x 16 px of a 128-channel
input: other shapes raise on the explicit entry and keep the 128x128 kernel
through conv_fwd_fp8r.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last
E4 = torch.float8_e4m3fn


def _C():
    from real_time_helmet_detection_amd.ops import _backend
    return _backend.require_ext()


def rel_err(got, want):
    got = got.detach().float().cpu()
    want = want.detach().float().cpu()
    denom = want.abs().max().clamp(min=1e-6)
    return ((got - want).abs().max() / denom).item()


def bits(t):
    return t.view(torch.uint8) if t.dtype == E4 else t


SHAPES = [
    # (B, Cin, Cout, H, W)
    (2, 128, 128, 16, 32),   # 2x2 tiles: every border kind, batch boundary
    (3, 128, 64, 8, 16),     # one tile per image, halo all outside, Cout < BN
    (1, 128, 256, 24, 48),   # an interior tile with no zero halo; two n blocks
    (1, 128, 40, 8, 16),     # Cout % 16 != 0: scalar e4m3 store, wide bf16
]
RAGGED = (1, 128, 128, 12, 20)
CIN256 = (1, 256, 128, 16, 32)


@functools.lru_cache(maxsize=None)
def _case(shape, k=3):
    """Inputs of one shape as test_conv_fwd_fp8_resident builds them (e4m3 x
    and skip, per-cout scaled e4m3 weights) and the fp32 conv on the
    dequantised values, computed once and shared by all modes. Every other
    image is scaled by 8, so a halo that leaks across an image border shows
    in the values."""
    b, cin, cout, h, w_ = shape
    g = torch.Generator().manual_seed(1000 * h + w_ + cin + cout)
    x = torch.randn(b, cin, h, w_, generator=g) * 0.5
    x = x * (8.0 ** (torch.arange(b) % 2)).view(-1, 1, 1, 1)
    x8 = x.to(E4)
    w = torch.randn(cout, cin, k, k, generator=g) * 0.1
    sw = w.abs().amax(dim=(1, 2, 3)).clamp(min=1e-8) / 240.0
    wq = w / sw.view(-1, 1, 1, 1)
    w8 = wq.to(E4).float() * sw.view(-1, 1, 1, 1)
    sk8 = (torch.randn(b, cout, h, w_, generator=g) * 0.5).to(E4)
    sc = torch.rand(cout, generator=g) + 0.5
    sh = torch.randn(cout, generator=g) * 0.1
    conv = F.conv2d(x8.float(), w8, None, padding=k // 2)
    return dict(x=x8.cuda().contiguous(memory_format=CL),
                skip=sk8.cuda().contiguous(memory_format=CL),
                wpk=_C().pack_weights_fp8(wq.cuda()), sc=(sc * sw).cuda(),
                sh=sh.cuda(), conv=conv, skip_f=sk8.float(), sc_f=sc, sh_f=sh)


def _want(c, mode):
    y = c['conv'] * c['sc_f'].view(1, -1, 1, 1) + c['sh_f'].view(1, -1, 1, 1)
    return F.relu(y + c['skip_f']) if mode == 'skip_relu' else y


def _args(c, mode, cout, out_fp8, k=3, stride=1):
    skip, act = (c['skip'], 1) if mode == 'skip_relu' else (None, 0)
    return (c['x'], c['wpk'], c['sc'], c['sh'], skip, k, k, stride, k // 2,
            cout, act, out_fp8)


@pytest.mark.parametrize('out_fp8', [True, False])
@pytest.mark.parametrize('mode', ['skip_relu', 'linear'])
@pytest.mark.parametrize('shape', SHAPES)
def test_conv_fwd_fp8r_halo(shape, mode, out_fp8):
    c = _case(shape)
    a = _args(c, mode, shape[2], out_fp8)
    n0 = _C().fp8_halo_launch_count()
    got = _C().conv_fwd_fp8r_halo(*a)
    assert _C().fp8_halo_launch_count() == n0 + 1
    ref = _C().conv_fwd_fp8r_tile128(*a)
    assert got.dtype == (E4 if out_fp8 else torch.bfloat16)
    err = rel_err(got.float(), _want(c, mode))
    print('fp8 halo %s %s out_fp8=%s: rel_err %.5f'
          % (shape, mode, out_fp8, err))
    assert got.float().abs().max().item() > 0
    assert torch.equal(bits(got), bits(ref))
    assert err < (0.08 if out_fp8 else 0.05)


@pytest.mark.parametrize('out_fp8', [True, False])
def test_conv_fwd_fp8r_halo_refusals(out_fp8):
    """The explicit entry refuses what the kernel cannot tile; conv_fwd_fp8r
    on the same inputs still equals the 128x128 kernel."""
    C = _C()
    cases = [
        (_case(RAGGED), 128, 3, 1),              # 12 x 20: ragged
        (_case(SHAPES[0], 1), 128, 1, 1),        # 1x1
        (_case(SHAPES[0]), 128, 3, 2),           # 3x3 stride 2
        (_case(CIN256), 128, 3, 1),              # Cin 256: two K blocks a tap
    ]
    for c, cout, k, stride in cases:
        a = _args(c, 'linear', cout, out_fp8, k, stride)
        n0 = C.fp8_halo_launch_count()
        with pytest.raises(RuntimeError):
            C.conv_fwd_fp8r_halo(*a)
        got = C.conv_fwd_fp8r(*a)
        assert C.fp8_halo_launch_count() == n0
        ref = C.conv_fwd_fp8r_tile128(*a)
        assert got.float().abs().max().item() > 0
        assert torch.equal(bits(got), bits(ref))
    c = _case(RAGGED)
    got = C.conv_fwd_fp8r(*_args(c, 'skip_relu', 128, out_fp8))
    assert rel_err(got.float(), _want(c, 'skip_relu')) < \
        (0.08 if out_fp8 else 0.05)


def test_conv_fwd_fp8r_dispatch(monkeypatch):
    """conv_fwd_fp8r on an eligible shape of 128 blocks: the first call
    decides (a measurement), the second runs the cached choice; both equal
    the 128x128 kernel. RTHD_FP8_HALO=0 keeps the halo kernel out,
    RTHD_NO_AUTOTUNE=1 takes the block-count heuristic, which picks it."""
    C = _C()
    monkeypatch.delenv('RTHD_FP8_HALO', raising=False)
    monkeypatch.delenv('RTHD_NO_AUTOTUNE', raising=False)
    c = _case((4, 128, 128, 64, 64))
    for mode in ('linear', 'skip_relu'):
        a = _args(c, mode, 128, True)
        ref = C.conv_fwd_fp8r_tile128(*a)
        assert ref.float().abs().max().item() > 0
        for _ in range(2):
            assert torch.equal(bits(C.conv_fwd_fp8r(*a)), bits(ref))
    a = _args(c, 'linear', 128, True)
    monkeypatch.setenv('RTHD_FP8_HALO', '0')
    n0 = C.fp8_halo_launch_count()
    ref = C.conv_fwd_fp8r_tile128(*a)
    assert torch.equal(bits(C.conv_fwd_fp8r(*a)), bits(ref))
    assert C.fp8_halo_launch_count() == n0
    monkeypatch.delenv('RTHD_FP8_HALO')
    monkeypatch.setenv('RTHD_NO_AUTOTUNE', '1')
    got = C.conv_fwd_fp8r(*a)
    assert C.fp8_halo_launch_count() == n0 + 1
    assert torch.equal(bits(got), bits(ref))


@functools.lru_cache(maxsize=None)
def _net():
    from real_time_helmet_detection_amd.models import StackedHourglass
    torch.manual_seed(41)
    net = StackedHourglass(1, 128, 6).cuda().to(memory_format=CL).eval()
    x = torch.randn(4, 3, 256, 256).cuda().contiguous(memory_format=CL)
    return net, x


def test_fp8_model_halo_equals_tile128(monkeypatch):
    """The fp8 serving forward (128-channel maps of 4 x 64^2, M = 16384) is
    the same bits with the halo kernel kept out and with the heuristic that
    takes it; only the second run launches it."""
    from real_time_helmet_detection_amd import amp
    C = _C()
    net, x = _net()

    def run():
        with torch.no_grad(), amp.autocast(True), amp.fp8_autocast(True):
            return net(x)

    monkeypatch.delenv('RTHD_NO_AUTOTUNE', raising=False)
    monkeypatch.setenv('RTHD_FP8_HALO', '0')
    n0 = C.fp8_halo_launch_count()
    ref = run()
    assert C.fp8_halo_launch_count() == n0
    monkeypatch.delenv('RTHD_FP8_HALO')
    monkeypatch.setenv('RTHD_NO_AUTOTUNE', '1')
    got = run()
    assert C.fp8_halo_launch_count() > n0
    assert torch.isfinite(ref.float()).all()
    assert ref.float().abs().max().item() > 0
    assert torch.equal(got, ref)


def test_fp8_graphed_predictor_equals_eager(monkeypatch):
    """One capture + replay of the fp8 serving graph with the new dispatch
    inside: boxes, classes and scores equal the ungraphed Prediction."""
    from real_time_helmet_detection_amd import amp
    from real_time_helmet_detection_amd.engine.evaluator import (
        Prediction, GraphedPredictor)
    monkeypatch.delenv('RTHD_FP8_HALO', raising=False)
    monkeypatch.delenv('RTHD_NO_AUTOTUNE', raising=False)
    net, x = _net()
    pred = Prediction(net, topk=20, scale_factor=4, conf_th=0.1, nms='nms',
                      nms_th=0.5).cuda()
    g = GraphedPredictor(pred, x.clone(), fp8=True, warmup=1)
    got = g(x)
    with torch.no_grad(), amp.autocast(True), amp.fp8_autocast(True):
        want = pred(x)
    n = 0
    for wl, gl in zip(want, got):
        assert len(wl) == len(gl) == x.shape[0]
        for wt, gt in zip(wl, gl):
            assert torch.equal(gt, wt)
            n += wt.numel()
    assert n > 0
