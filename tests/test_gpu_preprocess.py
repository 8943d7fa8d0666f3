"""GPU tests for the device-side serving preprocess
(ops/csrc/preprocess.hip): resize_u8 against the eager oracle
ops.eager.resize_images (itself Pillow-exact, tests/test_device_preprocess.py)
bit for bit, under graph capture, as the single-frame rthd::resize_frame, in
the raw-input export and in evaluate_step."""

import functools

import numpy as np
import pytest
import torch

from test_device_preprocess import (T_TREE, _bits, _make_voc_root,
                                    run_evaluate_step)

pytestmark = pytest.mark.gpu

CL = torch.channels_last

DTYPES = {'u8': (None, torch.float32),
          'f32': ('imagenet', torch.float32),
          'bf16': ('scratch', torch.bfloat16)}

# name -> (canvas (Hmax, Wmax), [(h, w), ...])
BATCHES = {
    'mixed': ((67, 131), [(67, 131), (1, 1), (16, 16), (9, 130), (64, 5)]),
    'mixed2': ((67, 131), [(5, 131), (67, 2), (33, 40), (66, 66), (24, 25)]),
    'wide': ((200, 260), [(200, 260)]),
    'identity': ((24, 24), [(24, 24)]),
    'empty': ((8, 8), []),
}
# (batch, T): T = 24 is no multiple of the 8-wide store group, puts a tile
# edge inside the image and mixes up- and downscale per axis; (200, 260) at
# 24 has ratios above 8 and bands wider than one pass of the block
CASES = [('mixed', 24), ('mixed', 40), ('wide', 24), ('identity', 24),
         ('empty', 24)]


def _hip():
    from real_time_helmet_detection_amd.ops import hip
    return hip


def _eager():
    from real_time_helmet_detection_amd.ops import eager
    return eager


@functools.lru_cache(maxsize=None)
def _batch(name):
    """Noise images in the corners of a canvas of 255s and random bytes."""
    (hmax, wmax), hw = BATCHES[name]
    g = torch.Generator().manual_seed(len(name) + hmax)
    canvas = torch.randint(0, 256, (len(hw), hmax, wmax, 3),
                           dtype=torch.uint8, generator=g)
    canvas[:, ::2] = 255
    for i, (h, w) in enumerate(hw):
        canvas[i, :h, :w] = torch.randint(0, 256, (h, w, 3),
                                          dtype=torch.uint8, generator=g)
    return canvas, torch.tensor(hw, dtype=torch.int32).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def _want(name, T, kind):
    canvas, sizes = _batch(name)
    pretrained, dtype = DTYPES[kind]
    return _eager().resize_images(canvas, sizes, T, pretrained, dtype)


def _assert_same(got, want, T, kind):
    B = want.shape[0]
    assert got.dtype == want.dtype and got.shape == want.shape
    if kind == 'u8':
        assert got.shape == (B, T, T, 3) and got.is_contiguous()
    else:
        assert got.shape == (B, 3, T, T)
        assert got.is_contiguous(memory_format=CL)
        if B:
            assert got.stride() == (T * T * 3, 1, T * 3, 3)
    assert torch.equal(_bits(got.cpu()), _bits(want))


@pytest.mark.parametrize('kind', ['u8', 'f32', 'bf16'])
@pytest.mark.parametrize('name,T', CASES)
def test_bitwise_parity(name, T, kind):
    canvas, sizes = _batch(name)
    pretrained, dtype = DTYPES[kind]
    got = _hip().resize_images(canvas.cuda(), sizes, T, pretrained, dtype)
    torch.cuda.synchronize()
    _assert_same(got, _want(name, T, kind), T, kind)


def test_cap_and_host_checks():
    from real_time_helmet_detection_amd.ops import functional as opsF
    hip = _hip()
    assert hip._C().resize_max_ratio() == opsF.RESIZE_MAX_RATIO == 16
    canvas, sizes = _batch('mixed')
    bad = sizes.clone()
    bad[0, 1] = 132
    with pytest.raises(ValueError):
        hip.resize_images(canvas.cuda(), bad, 24)
    # a canvas past 16 x T on one axis is refused, and the message says so
    tall = torch.zeros((1, 16 * 4 + 1, 4, 3), dtype=torch.uint8).cuda()
    with pytest.raises(RuntimeError, match='16'):
        hip.resize_images(tall, torch.tensor([[4, 4]], dtype=torch.int32), 4)
    torch.cuda.synchronize()


def test_captured_replay_equals_oracle():
    """Capture-legal: replayed from a graph on a batch copied in after the
    capture (other sizes, the same canvas shape), the call equals the
    oracle for the new batch."""
    T = 24
    hip = _hip()
    canvas, sizes = _batch('mixed')
    s_canvas, s_sizes = canvas.cuda(), sizes.cuda()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip.resize_images(s_canvas, s_sizes, T, 'imagenet')
    torch.cuda.current_stream().wait_stream(side)

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = hip.resize_images(s_canvas, s_sizes, T, 'imagenet')
    for name in ('mixed2', 'mixed'):
        canvas, sizes = _batch(name)
        s_canvas.copy_(canvas)
        s_sizes.copy_(sizes)
        graph.replay()
        torch.cuda.synchronize()
        _assert_same(out, _want(name, T, 'f32'), T, 'f32')


def test_resize_frame_op():
    T = 24
    hip = _hip()
    canvas, sizes = _batch('wide')
    (H, W), = sizes.tolist()
    dev = torch.device('cuda', torch.cuda.current_device())
    table = hip._norm_table(dev, 'imagenet', torch.float32)
    image, scale = torch.ops.rthd.resize_frame(canvas[0].cuda(), T, table)
    torch.cuda.synchronize()
    want = _want('wide', T, 'f32')
    _assert_same(image, want, T, 'f32')
    assert scale.dtype == torch.float32
    assert torch.equal(scale.cpu(), torch.tensor([W / T, H / T, W / T, H / T],
                                                 dtype=torch.float32))
    # rthd::resize_u8 is the batch form behind the dispatcher
    got = torch.ops.rthd.resize_u8(canvas.cuda(), sizes.cuda(), T, table)
    _assert_same(got, want, T, 'f32')


def test_raw_input_export_other_frame_size():
    """Trace with a 40 x 56 frame, run on a 72 x 48 one: nothing about the
    frame size is baked in. Boxes against the Python path to rtol 1e-5 (one
    fp32 multiply against resize_box_to_original_scale's float64 one)."""
    from real_time_helmet_detection_amd.engine.evaluator import (
        Prediction, resize_box_to_original_scale)
    from real_time_helmet_detection_amd.engine.exporter import (Export,
                                                                RawExport)
    from real_time_helmet_detection_amd.models import StackedHourglass
    T = 128
    torch.manual_seed(7)
    net = StackedHourglass(1, 32, 6).cuda().to(memory_format=CL).eval()
    ex = Export(net, topk=50, scale_factor=4, conf_th=0.05,
                nms_th=0.5).cuda().eval()
    raw = RawExport(ex, T, 'imagenet').cuda().eval()
    g = torch.Generator().manual_seed(5)
    traced_on = torch.randint(0, 256, (40, 56, 3), dtype=torch.uint8,
                              generator=g).cuda()
    frame = torch.randint(0, 256, (72, 48, 3), dtype=torch.uint8,
                          generator=g)
    with torch.no_grad():
        raw(traced_on)  # warms the conv inference caches
        traced = torch.jit.trace(raw, traced_on)
        boxes, clss, scores = traced(frame.cuda())
    assert 'rthd::resize_frame' in str(traced.inlined_graph)

    pred = Prediction(network=net, topk=50, scale_factor=4, conf_th=0.05,
                      nms='nms', nms_th=0.5).cuda().eval()
    image = _hip().resize_images(
        frame[None].cuda(), torch.tensor([[72, 48]], dtype=torch.int32), T,
        'imagenet')
    with torch.no_grad():
        box_l, cls_l, score_l = pred(image)
    want_boxes = resize_box_to_original_scale(
        box_l[0].cpu().numpy(), (48, 72), (T, T))
    assert boxes.shape[0] > 0 and boxes.shape == want_boxes.shape
    np.testing.assert_allclose(boxes.cpu().numpy().astype(np.float64),
                               want_boxes, rtol=1e-5, atol=0)
    assert torch.equal(clss.cpu(), cls_l[0].cpu())
    assert torch.equal(scores.cpu(), score_l[0].cpu())


def test_evaluate_step_gpu_flag_off_equals_on(tmp_path):
    from real_time_helmet_detection_amd.models import StackedHourglass
    root = _make_voc_root(tmp_path)
    torch.manual_seed(3)
    net = StackedHourglass(1, 32, 6).cuda().to(memory_format=CL).eval()
    dev = torch.device('cuda', torch.cuda.current_device())
    in_off, pred_off = run_evaluate_step(root, dev, False, net)
    in_on, pred_on = run_evaluate_step(root, dev, True, net)
    assert len(in_off) == len(in_on) == 2
    for a, b in zip(in_off, in_on):
        assert b.is_cuda and b.is_contiguous(memory_format=CL)
        assert a.shape == b.shape
        assert torch.equal(_bits(a.cpu()), _bits(b.cpu()))
    assert list(pred_off) == list(pred_on)
    for key in pred_off:
        assert pred_off[key].shape == pred_on[key].shape
