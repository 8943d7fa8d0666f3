"""GPU tests of rthd::nms_pack (the packed-emit instantiations of the kernels
in ops/csrc/nms.hip and soft_nms.hip): bit for bit against the existing
kernels (nms_batched / soft_nms_batched) plus gathers, which fixes both the
selection and the carried values."""

import functools

import pytest
import torch

from test_nms_pack import MODES, make_inputs

pytestmark = pytest.mark.gpu

CONF = 0.3
B = 3
# 63/64/65: one-word edge of the 64-candidate compaction; 200, 256: several
# words, pow2 and not; 1025: the global-mask branch of nms_kernel
SIZES = [1, 2, 63, 64, 65, 200, 256, 1025]


def _hip():
    from real_time_helmet_detection_amd.ops import hip
    return hip


def _bits(t):
    return t.contiguous().view(torch.int32)


def compose(mode, boxes, classes, scores, scale=None, conf=CONF):
    """The existing batched kernel of ``mode`` plus gathers -> packed."""
    hip = _hip()
    nb, n = scores.shape
    if mode == 'nms':
        idx, counts = hip.nms_batched(boxes, scores, 0.5, conf)
        kept = None
    else:
        idx, kept, counts = hip.soft_nms_batched(boxes, scores, 0.5, conf,
                                                 conf)
    out = torch.zeros(nb, 1 + n, 6, device=boxes.device)
    if scale is not None:
        scale = scale.reshape(-1, 4).expand(nb, 4)
    for i, k in enumerate(counts.tolist()):
        sel = idx[i, :k].long()
        b = boxes[i][sel]
        if scale is not None:
            b = b * scale[i]
        out[i, 0, 0] = k
        out[i, 1:1 + k, :4] = b
        out[i, 1:1 + k, 4] = scores[i][sel] if kept is None else kept[i, :k]
        out[i, 1:1 + k, 5] = classes[i][sel].float()
    return out, counts.tolist()


def pack(mode, boxes, classes, scores, scale=None, conf=CONF):
    return _hip().nms_pack(boxes, classes, scores, scale, MODES.index(mode),
                           0.5, 0.5, conf, conf)


def check(mode, boxes, classes, scores, scale=None, conf=CONF):
    got = pack(mode, boxes, classes, scores, scale, conf)
    want, counts = compose(mode, boxes, classes, scores, scale, conf)
    assert got.shape == want.shape and got.dtype == torch.float32
    assert torch.equal(_bits(got), _bits(want))
    return got, counts


@functools.lru_cache(maxsize=None)
def _inputs(n, seed=0):
    # more clusters with N, so that large N keeps a long output list
    return tuple(t.cuda() for t in
                 make_inputs(B, n, seed=seed + n, clusters=max(2, n // 6)))


SCALES = {
    'none': lambda: None,
    'vec': lambda: torch.tensor([1.5, 0.7, 1.5, 0.7]).cuda(),
    'per_image': lambda: (torch.arange(B * 4).reshape(B, 4).float() * 0.37
                          + 0.5).cuda(),
}


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('n', SIZES)
def test_bitwise_against_existing_kernel(mode, n):
    boxes, classes, scores = _inputs(n)
    for name, make in SCALES.items():
        got, counts = check(mode, boxes, classes, scores, make())
    if n >= 63:
        assert all(0 < k < n for k in counts)


@pytest.mark.parametrize('mode', MODES)
def test_cap_size_disjoint_boxes(mode):
    """N = 2048 = NMS_CAP, nothing overlaps: everything above conf is kept,
    so the compaction fills all 32 words."""
    n = 2048
    i = torch.arange(n)
    x = (i % 64).float() * 10
    y = (i // 64).float() * 10
    one = torch.stack([x, y, x + 8, y + 8], dim=1)
    boxes = torch.stack([one, one + 1, one.flip(0)]).cuda()
    g = torch.Generator().manual_seed(11)
    scores = torch.rand(B, n, generator=g).cuda()
    scores[1] = scores[1] * 0.5 + 0.5  # image 1: all above conf
    classes = torch.randint(0, 2, (B, n), generator=g).cuda()
    got, counts = check(mode, boxes, classes, scores, SCALES['vec']())
    assert counts[1] == n
    assert counts[0] == int((scores[0] >= CONF).sum())


@pytest.mark.parametrize('mode', MODES)
def test_all_below_and_all_kept(mode):
    boxes, classes, scores = (t.clone() for t in _inputs(65))
    scores[0] = scores[0] * CONF * 0.9          # image 0: nothing passes
    i = torch.arange(65, device='cuda').float() * 50
    boxes[2] = torch.stack([i, i, i + 20, i + 20], dim=1)
    scores[2] = scores[2] * 0.5 + 0.5           # image 2: all kept
    got, counts = check(mode, boxes, classes, scores)
    assert counts[0] == 0 and counts[2] == 65
    assert torch.count_nonzero(got[0]) == 0
    assert got[2, 0, 0] == 65


@pytest.mark.parametrize('mode', MODES)
def test_score_ties_and_identical_boxes(mode):
    boxes, classes, scores = (t.clone() for t in _inputs(200))
    scores = (scores * 4).floor() / 4 + 0.125   # five distinct values
    boxes[1] = boxes[1, :1]                     # image 1: one box 200 times
    got, counts = check(mode, boxes, classes, scores)
    if mode == 'nms':
        assert counts[1] == 1


def test_empty():
    boxes, classes, scores = (t.cuda() for t in make_inputs(B, 0))
    for mode in MODES:
        got = pack(mode, boxes, classes, scores)
        assert got.shape == (B, 1, 6) and got.is_cuda
        assert torch.count_nonzero(got) == 0


def test_above_cap_refused_by_op_served_by_eager():
    from real_time_helmet_detection_amd import ops
    n = 2049
    boxes, classes, scores = (t.cuda() for t in make_inputs(1, n, seed=5))
    scores[:, 24:] *= CONF * 0.9  # few pass conf: the eager loop stays short
    with pytest.raises(RuntimeError, match='cap'):
        torch.ops.rthd.nms_pack(boxes, classes, scores, None, 0, 0.5, 0.5,
                                CONF, CONF)
    for mode in MODES:
        got = ops.nms_pack(boxes, classes, scores, None, MODES.index(mode),
                           0.5, 0.5, CONF, CONF)
        want = ops.eager.nms_pack(boxes.cpu(), classes.cpu(), scores.cpu(),
                                  None, MODES.index(mode), 0.5, 0.5, CONF,
                                  CONF)
        assert got.is_cuda and got.shape == (1, n + 1, 6)
        assert got[0, 0, 0].item() == want[0, 0, 0].item() > 0
        torch.testing.assert_close(got.cpu(), want, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize('mode', MODES)
def test_graph_capture_replays_on_new_inputs(mode):
    first = _inputs(200)
    second = _inputs(200, seed=9)
    scale = SCALES['vec']()
    static = [t.clone() for t in first]
    pack(mode, *static, scale)  # loads the kernel outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pack(mode, *static, scale)
    for inputs in (second, first):
        for dst, src in zip(static, inputs):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(out), _bits(pack(mode, *inputs, scale)))
    assert not torch.equal(pack(mode, *first, scale),
                           pack(mode, *second, scale))
