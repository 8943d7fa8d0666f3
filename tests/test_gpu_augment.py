"""GPU tests for the device-side train augmentation (ops/csrc/augment.hip):
augment_u8_kernel against the eager oracle ops.eager.augment_images bit for
bit, under graph capture, and feeding the graphed training step."""

import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CL = torch.channels_last

HMAX, WMAX = 40, 56
SIZES_HW = [(40, 56), (33, 47), (24, 24)]
DTYPES = {'u8': (None, torch.float32),
          'f32': ('imagenet', torch.float32),
          'bf16': ('scratch', torch.bfloat16)}


def _hip():
    from real_time_helmet_detection_amd.ops import hip
    return hip


def _eager():
    from real_time_helmet_detection_amd.ops import eager
    return eager


@functools.lru_cache(maxsize=None)
def _canvas():
    """Three noise images in the corners of a 40 x 56 canvas whose padding
    is 255: reading it would show."""
    g = torch.Generator().manual_seed(0)
    img = torch.full((3, HMAX, WMAX, 3), 255, dtype=torch.uint8)
    for i, (h, w) in enumerate(SIZES_HW):
        img[i, :h, :w] = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8,
                                       generator=g)
    return img, torch.tensor(SIZES_HW, dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def _coef_sets(T):
    """name -> (3,5) fp32: sample_params draws and hand-made extremes."""
    from real_time_helmet_detection_amd.data.augment import (
        AugParams, TrainAugmentor, map_coefficients)
    sizes_wh = [(w, h) for h, w in SIZES_HW]

    def rows(params):
        c = [list(map_coefficients(p, wh, T)) + [p.factor]
             for p, wh in zip(params, sizes_wh)]
        return torch.tensor(c, dtype=torch.float64).float()

    sets = {}
    aug = TrainAugmentor(multiscale=(T, T, 64), seed=100 + T)
    for k in range(4):
        params, target = aug.sample_params(sizes_wh)
        assert target == T
        sets['sampled%d' % k] = rows(params)
    # maximum translate is 0.1 of the side
    sets['scale_half'] = rows([
        AugParams(1.5, 0.5, 0.1 * w, -0.1 * h, 0, 0, 0, 0, False)
        for w, h in sizes_wh])
    sets['scale_1p5'] = rows([
        AugParams(1.2, 1.5, -0.1 * w, 0.1 * h, h // 10, 0, 0, w // 10, False)
        for w, h in sizes_wh])
    sets['flip'] = rows([
        AugParams(1.0, 1.0, 0.0, 0.0, 0, 0, 0, 0, True) for _ in sizes_wh])
    # every source coordinate far outside: all black, far enough (up to
    # an fp32 overflow to +inf in the last row) that the clamp ahead of the
    # int cast is what keeps the index sane
    sets['outside'] = torch.tensor([[1.0, 1e4, 1.0, 0.0, 1.3],
                                    [1.0, 0.0, 1.0, -3e9, 1.3],
                                    [-5e8, -70.0, 3e38, 3e38, 1.3]])
    return sets


@functools.lru_cache(maxsize=None)
def _want(T, name, kind):
    img, sizes = _canvas()
    pretrained, dtype = DTYPES[kind]
    return _eager().augment_images(img, sizes, _coef_sets(T)[name], T,
                                   pretrained, dtype)


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16,
                   4: torch.int32}[t.element_size()])


def _assert_same(got, want, T, kind):
    assert got.dtype == want.dtype and got.shape == want.shape
    if kind == 'u8':
        assert got.shape == (3, T, T, 3) and got.is_contiguous()
    else:
        assert got.shape == (3, 3, T, T)
        assert got.is_contiguous(memory_format=CL)
        assert got.stride() == (T * T * 3, 1, T * 3, 3)
    assert torch.equal(_bits(got.cpu()), _bits(want))


@pytest.mark.parametrize('kind', ['u8', 'f32', 'bf16'])
@pytest.mark.parametrize('T', [32, 20, 64])
def test_bitwise_parity(T, kind):
    """T = 20: the row tail (bf16 groups of 8) and, for bf16 and uint8,
    rows off the vector-store grid."""
    img, sizes = _canvas()
    pretrained, dtype = DTYPES[kind]
    img_d = img.cuda()
    for name, coef in _coef_sets(T).items():
        got = _hip().augment_images(img_d, sizes, coef, T, pretrained, dtype)
        torch.cuda.synchronize()
        want = _want(T, name, kind)
        _assert_same(got, want, T, kind)
        if name == 'outside':  # all black, in the oracle and so here
            assert not _want(T, name, 'u8').any()


@pytest.mark.parametrize('kind', ['u8', 'bf16'])
def test_odd_storage_offset_and_device_args(kind):
    """A contiguous input view that starts at an odd byte, with sizes and
    coefficients already on the device."""
    T = 20
    img, sizes = _canvas()
    pretrained, dtype = DTYPES[kind]
    flat = torch.cat([torch.zeros(3, dtype=torch.uint8), img.reshape(-1)])
    view = flat.cuda()[3:].view(3, HMAX, WMAX, 3)
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    coef = _coef_sets(T)['sampled0']
    got = _hip().augment_images(view, sizes.cuda(), coef.cuda(), T,
                                pretrained, dtype)
    torch.cuda.synchronize()
    _assert_same(got, _want(T, 'sampled0', kind), T, kind)


def test_host_checks():
    img, sizes = _canvas()
    img_d = img.cuda()
    coef = _coef_sets(32)['sampled0']
    hip = _hip()
    bad = sizes.clone()
    bad[1, 0] = HMAX + 1
    with pytest.raises(ValueError):
        hip.augment_images(img_d, bad, coef, 32)
    bad = sizes.clone()
    bad[2, 1] = 0
    with pytest.raises(ValueError):
        hip.augment_images(img_d, bad, coef, 32)
    nan = coef.clone()
    nan[0, 1] = float('inf')
    with pytest.raises(ValueError):
        hip.augment_images(img_d, sizes, nan, 32)
    with pytest.raises(ValueError):
        hip.augment_images(img_d, sizes, coef, 0)
    with pytest.raises(ValueError):
        hip.augment_images(img_d, sizes, coef, 32, 'imagenet', torch.float16)
    with pytest.raises(RuntimeError):  # the extension's own shape checks
        hip.augment_images(img_d, sizes.cuda()[:2], coef.cuda(), 32)
    with pytest.raises(RuntimeError):
        hip.augment_images(img_d.float(), sizes.cuda(), coef.cuda(), 32)
    torch.cuda.synchronize()


def test_captured_replay_equals_eager():
    """Capture-legal: the call replayed from a graph, on inputs swapped in
    after the capture, equals the plain launch and the oracle."""
    T = 20
    img, sizes = _canvas()
    sets = _coef_sets(T)
    s_img = img.cuda()
    s_sizes = sizes.cuda()
    s_coef = sets['sampled0'].cuda()
    hip = _hip()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip.augment_images(s_img, s_sizes, s_coef, T, 'scratch',
                           torch.bfloat16)
    torch.cuda.current_stream().wait_stream(side)

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = hip.augment_images(s_img, s_sizes, s_coef, T, 'scratch',
                                 torch.bfloat16)
    for name in ('sampled1', 'scale_1p5', 'sampled0'):
        s_coef.copy_(sets[name])
        graph.replay()
        torch.cuda.synchronize()
        plain = hip.augment_images(s_img, s_sizes, s_coef, T, 'scratch',
                                   torch.bfloat16)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(plain))
        _assert_same(out, _want(T, name, 'bf16'), T, 'bf16')


def test_graphed_train_step_device_augmented_batch():
    """One GraphedTrainStep on a 64 x 64, B = 2 batch prepared by
    trainer.prepare_batch on the device (augment_u8_kernel + encode_targets
    ahead of the replay) and by the eager oracle on the host. The images
    must agree bit for bit; the targets within the heatmap tolerance of
    tests/test_gpu_encode.py (5e-6: the device exponential); the losses
    within the graphed-versus-eager tolerance of tests/test_gpu_e2e.py
    (rtol 0.05, atol 0.5)."""
    from real_time_helmet_detection_amd.config import build_parser
    from real_time_helmet_detection_amd.data import (SyntheticVOC,
                                                     TrainAugmentor)
    from real_time_helmet_detection_amd.engine.graphed import \
        GraphedTrainStep
    from real_time_helmet_detection_amd.engine.trainer import prepare_batch
    from real_time_helmet_detection_amd.loss import LossCalculator
    from real_time_helmet_detection_amd.models import StackedHourglass

    args = build_parser(['--train-flag', '--amp', '--device-augment'])
    ds = SyntheticVOC(
        transform=TrainAugmentor(multiscale=(64, 64, 64), seed=3), size=2,
        imsize=64, seed=5)
    raw = ds.collate_device_aug([ds[0], ds[1]])[:6]
    img_u8, sizes, coef, T, boxes, labels = raw
    assert T == 64 and (labels >= 0).any()
    dev = torch.device('cuda', torch.cuda.current_device())

    device_batch = prepare_batch(raw, dev, args, True, True)
    torch.cuda.synchronize()
    eager = _eager()
    host_batch = (
        eager.augment_images(img_u8, sizes, coef, T, args.pretrained,
                             torch.bfloat16),
        *eager.encode_targets(boxes, labels, (T, T), args.scale_factor,
                              args.num_cls, args.normalized_coord))
    assert device_batch[0].dtype == torch.bfloat16
    assert device_batch[0].is_contiguous(memory_format=CL)
    assert torch.equal(_bits(device_batch[0].cpu()), _bits(host_batch[0]))
    for d, h in zip(device_batch[1:], host_batch[1:]):
        torch.testing.assert_close(d.cpu(), h, rtol=0, atol=5e-6)
    assert host_batch[4].sum() > 0

    torch.manual_seed(41)
    net0 = StackedHourglass(1, 32, 6).cuda().to(memory_format=CL)

    def run(batch):
        net = copy.deepcopy(net0).train()
        calc = LossCalculator().cuda()
        opt = torch.optim.Adam(net.parameters(), lr=1e-3, fused=True,
                               capturable=True)
        g = GraphedTrainStep(net, calc, opt, num_cls=2,
                             normalized_coord=False, amp_on=True)
        assert g.step(*batch) is not None, 'graph capture failed'
        assert g.enabled and len(g.graphs) == 1
        return calc.get_loss_log()

    host = run(tuple(t.cuda() for t in host_batch))
    device = run(device_batch)
    for key in ('hm', 'offset', 'size', 'total'):
        print(key, 'host', host[key], 'device', device[key])
        assert len(device[key]) == 1 and np.isfinite(device[key]).all()
        torch.testing.assert_close(torch.tensor(device[key]),
                                   torch.tensor(host[key]),
                                   rtol=0.05, atol=0.5)
