"""GPU tests of --infer-dtype in evaluate_step: bf16 is the predictor under
amp.autocast, fp32 is the path without the flag."""

import numpy as np
import pytest
import torch

from real_time_helmet_detection_amd.config import build_parser

pytestmark = pytest.mark.gpu

T = 128
ARGV = ['--imsize', str(T), '--conf-th', '0.05', '--batch-size', '2']


@pytest.fixture(autouse=True)
def _heuristic_variants(monkeypatch):
    monkeypatch.setenv('RTHD_NO_AUTOTUNE', '1')


def _setup():
    from real_time_helmet_detection_amd.data import SyntheticVOC, \
        TestAugmentor
    from real_time_helmet_detection_amd.engine.evaluator import Prediction
    from real_time_helmet_detection_amd.models import StackedHourglass
    torch.manual_seed(3)
    net = StackedHourglass(1, 32, 6).cuda() \
        .to(memory_format=torch.channels_last).eval()
    pred = Prediction(network=net, topk=20, scale_factor=4, conf_th=0.05,
                      nms='nms', nms_th=0.5).cuda().eval()
    ds = SyntheticVOC(transform=TestAugmentor(T), imsize=T, size=4)
    loader = torch.utils.data.DataLoader(
        ds, batch_size=2, shuffle=False, num_workers=0,
        collate_fn=ds.collate_fn)
    return pred, loader


def _step(pred, loader, args):
    from real_time_helmet_detection_amd.engine.evaluator import evaluate_step
    dev = torch.device('cuda', torch.cuda.current_device())
    return evaluate_step(loader, pred, dev, args)


def _same(a, b):
    assert list(a) == list(b) and len(a) == 4
    assert any(len(v) for v in a.values())
    for key in a:
        assert a[key].shape == b[key].shape
        assert np.array_equal(a[key], b[key])


def test_bf16_equals_autocast_by_hand():
    from real_time_helmet_detection_amd import amp
    pred, loader = _setup()
    got = _step(pred, loader, build_parser(ARGV + ['--infer-dtype', 'bf16']))
    seen = []
    pred.register_forward_pre_hook(
        lambda m, inp: seen.append(amp.is_autocast_enabled()))
    with amp.autocast(True):
        want = _step(pred, loader, build_parser(ARGV))
    assert seen == [True, True]
    _same(got, want)
    fp32 = _step(pred, loader, build_parser(ARGV))
    assert any(not np.array_equal(fp32[k], got[k]) for k in got), \
        'bf16 run indistinguishable from fp32: the flag did nothing'


def test_fp32_equals_flag_absent():
    from real_time_helmet_detection_amd import amp
    pred, loader = _setup()
    seen = []
    pred.register_forward_pre_hook(
        lambda m, inp: seen.append(amp.is_autocast_enabled()))
    got = _step(pred, loader, build_parser(ARGV + ['--infer-dtype', 'fp32']))
    args = build_parser(ARGV)
    del args.infer_dtype  # a namespace from before the flag existed
    want = _step(pred, loader, args)
    assert seen == [False] * 4
    _same(got, want)
