"""GPU tests of the serving export (engine/exporter.py ServeExport and
export_model's infer_dtype): the saved trace against the live modules and
against the matching Export trace, and its replay from a captured graph."""

import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

CL = torch.channels_last
TOL = dict(atol=2e-2, rtol=2e-2)  # trace against live, as
#                                   test_native_traced_export_parity

# dtype -> (hourglass width, imsize). fp8 needs cin % 128 == 0 and at least
# 16384 pixels per conv to reach the e4m3 kernel (ops/hip.py conv_bn_act)
NETS = {'fp32': (32, 128), 'bf16': (32, 128), 'fp8': (128, 512)}


@pytest.fixture(autouse=True)
def _heuristic_variants(monkeypatch):
    # live and traced runs take the same conv variant
    monkeypatch.setenv('RTHD_NO_AUTOTUNE', '1')


def _frames(T, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda h, w: torch.randint(0, 256, (h, w, 3), dtype=torch.uint8,
                                    generator=g).cuda()
    # neither has the traced (T, T) size
    return mk(T + 24, T - 16), mk(T + 24, T - 16)


@pytest.fixture(scope='module')
def root(tmp_path_factory):
    return str(tmp_path_factory.mktemp('serve_export'))


@functools.lru_cache(maxsize=None)
def _exported(root, dtype, nms='nms', flip=False):
    """One export per configuration, shared by the tests below."""
    from real_time_helmet_detection_amd.engine.exporter import (
        Export, RawExport, ServeExport, export_model)
    from real_time_helmet_detection_amd.models import StackedHourglass
    width, T = NETS[dtype]
    torch.manual_seed(7)
    net = StackedHourglass(1, width, 6).cuda().to(memory_format=CL).eval()
    ex = Export(net, topk=50, scale_factor=4, conf_th=0.05, nms_th=0.5,
                nms=nms, flip_test=flip).cuda().eval()
    serve = ServeExport(ex, T, 'imagenet')
    save = os.path.join(root, '%s_%s_%d' % (dtype, nms, flip))
    paths = export_model(ex, save_dir=save, imsize=T, do_gpu=True,
                         raw_input=True, infer_dtype=dtype, serve=serve)
    live = RawExport(ex.cuda(), T, 'imagenet').cuda().eval()
    return paths, live, T


def _compare(packed, boxes, clss, scores):
    from real_time_helmet_detection_amd import ops
    assert packed.dim() == 2 and packed.shape[1] == 6
    (b,), (c,), (s,) = ops.unpack_detections(packed)
    print('detections: serve %d, other %d' % (b.shape[0], boxes.shape[0]))
    assert b.shape[0] == boxes.shape[0] > 0
    assert torch.count_nonzero(packed[1 + b.shape[0]:]) == 0
    torch.testing.assert_close(b, boxes.float(), **TOL)
    torch.testing.assert_close(s, scores.float(), **TOL)
    assert torch.equal(c, clss)


@pytest.mark.parametrize('dtype', ['fp32', 'bf16', 'fp8'])
def test_serving_trace_against_live(root, dtype):
    from real_time_helmet_detection_amd import amp
    paths, live, T = _exported(root, dtype)
    suffix = '' if dtype == 'fp32' else '_' + dtype
    for key, stem in (('gpu', 'gpu'), ('gpu_raw', 'gpu_raw'),
                      ('gpu_serve', 'gpu_serve')):
        assert os.path.basename(paths[key]) == \
            'jit_traced_model_%s%s.pth' % (stem, suffix)
    assert os.path.basename(paths['cpu']) == 'jit_traced_model_cpu.pth'

    loaded = torch.jit.load(paths['gpu_serve'])
    graph = loaded.inlined_graph
    text = str(graph)
    assert 'rthd::nms_pack' in text and 'rthd::resize_frame' in text
    consts = [n.output().toIValue()
              for n in graph.findAllNodes('prim::Constant')
              if n.output().type().kind() == 'TensorType']
    dtypes = {t.dtype for t in consts if t is not None}
    if dtype == 'fp8':
        assert 'rthd::conv_fwd_fp8r' in text
    if dtype == 'bf16':
        assert torch.bfloat16 in dtypes, 'no bf16 packed weights baked in'
    if dtype == 'fp32':
        assert torch.bfloat16 not in dtypes

    frame, _ = _frames(T, 5)
    with torch.no_grad():
        packed = loaded(frame)  # no autocast state in the consumer
        with amp.infer_context(dtype):
            boxes, clss, scores = live(frame)
    assert packed.shape == (1 + 50, 6) and packed.dtype == torch.float32
    _compare(packed, boxes, clss, scores)


@pytest.mark.parametrize('nms,flip', [('nms', False), ('soft-nms', False),
                                      ('nms', True)])
def test_serving_trace_against_export_trace(root, nms, flip):
    paths, _, T = _exported(root, 'fp32', nms, flip)
    serve = torch.jit.load(paths['gpu_serve'])
    raw = torch.jit.load(paths['gpu_raw'])
    if flip:
        assert 'rthd::decode_logits' in str(serve.inlined_graph)
    frame, _ = _frames(T, 6)
    with torch.no_grad():
        _compare(serve(frame), *raw(frame))


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_serving_trace_replays_from_a_graph(root, dtype):
    paths, _, T = _exported(root, dtype)
    loaded = torch.jit.load(paths['gpu_serve'])
    first, second = _frames(T, 8)
    static = first.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(3):  # the TorchScript executor settles
            loaded(static)
    torch.cuda.current_stream().wait_stream(side)
    with torch.no_grad():
        want = [loaded(first).clone(), loaded(second).clone()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        out = loaded(static)
    for frame, w in ((second, want[1]), (first, want[0])):
        static.copy_(frame)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), w.view(torch.int32))
    assert want[0][0, 0] > 0 and not torch.equal(want[0], want[1])


def test_fp32_export_without_serve_writes_todays_files(tmp_path):
    from real_time_helmet_detection_amd.engine.exporter import (Export,
                                                                export_model)
    from real_time_helmet_detection_amd.models import StackedHourglass
    torch.manual_seed(7)
    net = StackedHourglass(1, 32, 6).cuda().to(memory_format=CL).eval()
    ex = Export(net, topk=50, scale_factor=4, conf_th=0.05,
                nms_th=0.5).cuda().eval()
    paths = export_model(ex, save_dir=str(tmp_path), imsize=128, do_gpu=True,
                         infer_dtype='fp32')
    assert sorted(os.listdir(tmp_path)) == ['jit_traced_model_cpu.pth',
                                            'jit_traced_model_gpu.pth']
    assert sorted(paths) == ['cpu', 'gpu']
    paths = export_model(ex, save_dir=str(tmp_path), imsize=128, do_gpu=True,
                         raw_input=True)
    assert sorted(os.listdir(tmp_path)) == [
        'jit_traced_model_cpu.pth', 'jit_traced_model_gpu.pth',
        'jit_traced_model_gpu_raw.pth']
