"""The soft-NMS kernel (ops/csrc/soft_nms.hip) against the CPU eager oracle:
eager.soft_nms on the candidates with score >= conf_th.

Indices and counts must match exactly; scores to rtol 2e-5. That is 5x
under the 1e-4 margins every parity case is validated for by the float64
simulator of tests/test_soft_nms.py (so the order cannot flip within
tolerance) and about 30x over the fp32 error of the eager oracle itself (a
few ulp per overlapping round from expf and the IoU quotient, about ten
overlapping rounds per cluster).
"""

import math
import os

import pytest
import torch

from real_time_helmet_detection_amd import ops
from real_time_helmet_detection_amd.ops import eager

from test_soft_nms import (SIGMA, SCORE_TH, MARGIN, clustered_boxes,
                           case_margins, first_valid, parity_case,
                           batch_case, per_image_oracle, check_batched)

pytestmark = pytest.mark.gpu

RTOL = 2e-5
CL = torch.channels_last


def run_batched(boxes, scores, sigma, score_th, conf_th):
    got = ops.soft_nms_batched(boxes.cuda(), scores.cuda(), sigma, score_th,
                               conf_th)
    assert all(t.is_cuda for t in got)
    return got


@pytest.mark.parametrize('n', (1, 2, 63, 64, 65, 200, 256))
def test_kernel_matches_eager(n):
    """Worst relative score error measured on MI355X over these cases:
    2.5e-07 (N=200; 1.1e-07 at N=63, 9.2e-08 at N=64, 1.1e-07 at N=65,
    2.2e-07 at N=256, 0 at N=1 and 2), i.e. about 80x under RTOL."""
    boxes, scores, keep, _, _ = parity_case(n)
    want = per_image_oracle(boxes[None], scores[None], SIGMA, SCORE_TH,
                            SCORE_TH)
    assert want[0][0].tolist() == keep  # oracle agrees with the simulator
    got = run_batched(boxes[None], scores[None], SIGMA, SCORE_TH, SCORE_TH)
    assert got[0].shape == (1, n) and got[1].shape == (1, n)
    worst = check_batched(got, want, RTOL)
    print('N=%d worst relative score error %.3g' % (n, worst))


def test_batch_of_three_with_an_empty_image():
    boxes, scores, conf_th = batch_case(65)
    want = per_image_oracle(boxes, scores, SIGMA, conf_th, conf_th)
    got = run_batched(boxes, scores, SIGMA, conf_th, conf_th)
    counts = got[2].tolist()
    assert counts[2] == 0 and len(set(counts)) == 3, counts
    worst = check_batched(got, want, RTOL)
    print('B=3 worst relative score error %.3g' % worst)


def test_no_candidates():
    idx, sc, counts = ops.soft_nms_batched(
        torch.zeros(2, 0, 4, device='cuda'), torch.zeros(2, 0, device='cuda'),
        SIGMA, SCORE_TH, SCORE_TH)
    assert idx.shape == (2, 0) and sc.shape == (2, 0)
    assert counts.tolist() == [0, 0]
    keep, rescored = ops.soft_nms(torch.zeros(0, 4, device='cuda'),
                                  torch.zeros(0, device='cuda'),
                                  sigma=SIGMA, score_th=SCORE_TH)
    assert keep.numel() == 0 and rescored.numel() == 0
    assert keep.dtype == torch.long


def disjoint_grid(cols, rows, side=6.0, pitch=8.0):
    ys, xs = torch.meshgrid(torch.arange(rows), torch.arange(cols),
                            indexing='ij')
    x1 = xs.reshape(-1).float() * pitch
    y1 = ys.reshape(-1).float() * pitch
    return torch.stack([x1, y1, x1 + side, y1 + side], dim=1)


def test_exact_ties_go_to_the_lowest_index():
    # disjoint boxes: every weight is exp(0) == 1, so the result is exact
    boxes = disjoint_grid(8, 8)
    levels = torch.tensor([0.3, 0.9, 0.5, 0.7])
    scores = levels[torch.arange(64) % 4]
    idx, sc, counts = run_batched(boxes[None], scores[None], SIGMA, 0.1, 0.1)
    order = sorted(range(64), key=lambda i: (-scores[i].item(), i))
    assert counts.tolist() == [64]
    assert idx[0].tolist() == order
    assert torch.equal(sc[0].cpu(), scores[order])


def test_identical_boxes():
    boxes = torch.tensor([[10., 10., 50., 60.]]).repeat(8, 1)
    scores = torch.full((8,), 0.9)
    idx, sc, counts = run_batched(boxes[None], scores[None], SIGMA, 0.05,
                                  0.05)
    assert counts.tolist() == [2]
    assert idx[0, :2].tolist() == [0, 1]
    want = torch.tensor([0.9, 0.9 * math.exp(-2.0)])
    torch.testing.assert_close(sc[0, :2].cpu(), want, rtol=RTOL, atol=0)
    assert not sc[0, 2:].any() and not idx[0, 2:].any()


def test_zero_area_boxes_never_decay_anything():
    def make(seed):
        boxes, scores = clustered_boxes(65, seed)
        boxes = boxes.clone()
        boxes[::5, 2] = boxes[::5, 0]          # zero width
        boxes[2::7, 3] = boxes[2::7, 1] - 3.0  # negative height
        return boxes, scores
    boxes, scores, keep, _, _ = first_valid(make, SCORE_TH, 'zero-area')
    want = per_image_oracle(boxes[None], scores[None], SIGMA, SCORE_TH,
                            SCORE_TH)
    got = run_batched(boxes[None], scores[None], SIGMA, SCORE_TH, SCORE_TH)
    check_batched(got, want, RTOL)
    # a degenerate box overlaps nothing: it is selected with its own score
    k = int(got[2][0])
    sel = got[0][0, :k].cpu().long()
    degenerate = torch.zeros(65, dtype=torch.bool)
    degenerate[::5] = True
    degenerate[2::7] = True
    live = degenerate & (scores >= SCORE_TH)
    pos = {int(j): i for i, j in enumerate(sel.tolist())}
    for j in live.nonzero().squeeze(1).tolist():
        assert got[1][0, pos[j]].item() == scores[j].item()


def test_cap_2048_disjoint_is_exact():
    boxes = disjoint_grid(64, 32)
    g = torch.Generator().manual_seed(0)
    scores = torch.linspace(0.05, 1.0, 2048)[torch.randperm(2048,
                                                            generator=g)]
    th = 0.1
    idx, sc, counts = run_batched(boxes[None], scores[None], SIGMA, th, 0.0)
    order = torch.argsort(scores, descending=True)
    order = order[scores[order] > th]
    k = order.numel()
    assert 0 < k < 2048 and counts.tolist() == [k]
    assert torch.equal(idx[0, :k].cpu().long(), order)
    assert torch.equal(sc[0, :k].cpu(), scores[order])
    assert not sc[0, k:].any() and not idx[0, k:].any()


def test_above_the_cap_falls_back_to_eager():
    # 2049 candidates, about forty of them at or above conf_th
    conf_th = 0.98
    boxes, scores, keep, _, _ = parity_case(2049, conf_th)
    assert 8 < len(keep)
    want = per_image_oracle(boxes[None], scores[None], SIGMA, SCORE_TH,
                            conf_th)
    got = run_batched(boxes[None], scores[None], SIGMA, SCORE_TH, conf_th)
    check_batched(got, want, RTOL)


def test_single_image_entry():
    boxes, scores, _, _, _ = parity_case(65)
    sel = (scores >= SCORE_TH).nonzero().squeeze(1)
    b, s = boxes[sel], scores[sel]
    want_keep, want_sc = eager.soft_nms(b, s, sigma=SIGMA, score_th=SCORE_TH)
    keep, sc = ops.soft_nms(b.cuda(), s.cuda(), sigma=SIGMA,
                            score_th=SCORE_TH)
    assert keep.is_cuda and keep.dtype == torch.long
    assert keep.tolist() == want_keep.tolist()
    torch.testing.assert_close(sc.cpu(), want_sc, rtol=RTOL, atol=0)


def test_eager_override_still_selects_eager(monkeypatch):
    boxes, scores, _, _, _ = parity_case(65)
    monkeypatch.setenv('RTHD_EAGER_GPU', '1')
    got = run_batched(boxes[None], scores[None], SIGMA, SCORE_TH, SCORE_TH)
    want = per_image_oracle(boxes[None], scores[None], SIGMA, SCORE_TH,
                            SCORE_TH)
    check_batched(got, want, RTOL)


def test_graph_capture_and_replay():
    b0, s0, _, _, _ = parity_case(65)
    b1, s1, _, _, _ = parity_case(63)
    warm_b = torch.stack([b0, b0]).cuda()
    warm_s = torch.stack([s0, s0]).cuda()
    static_b, static_s = warm_b.clone(), warm_s.clone()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.soft_nms_batched(static_b, static_s, SIGMA, SCORE_TH, SCORE_TH)
    torch.cuda.current_stream().wait_stream(side)

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.soft_nms_batched(static_b, static_s, SIGMA, SCORE_TH,
                                   SCORE_TH)

    # different valid inputs: image 0 = the N=63 case padded with two
    # sub-threshold candidates, image 1 = the N=65 case reversed
    pad_b = torch.cat([b1, torch.zeros(2, 4)])
    pad_s = torch.cat([s1, torch.zeros(2)])
    new_b = torch.stack([pad_b, b0.flip(0)])
    new_s = torch.stack([pad_s, s0.flip(0)])
    for i in range(2):
        _, _, ma, mb = case_margins(new_b[i], new_s[i], SCORE_TH)
        assert ma >= MARGIN and mb >= MARGIN
    static_b.copy_(new_b)
    static_s.copy_(new_s)
    graph.replay()
    torch.cuda.synchronize()
    want = per_image_oracle(new_b, new_s, SIGMA, SCORE_TH, SCORE_TH)
    check_batched(out, want, RTOL)


# seed and topk of the Prediction case below; at this seed both images keep
# simulator margins well above MARGIN on the decoded boxes
PRED_SEED = 0
PRED_TOPK = 20
PRED_CONF = 0.05


class SpreadHeads(torch.nn.Module):
    """The tiny net with an affine map on its raw output. An untrained net
    puts every peak score within 0.02 of the others and decodes boxes a
    pixel wide, which leaves soft-NMS nothing to do and no margin between
    candidates; this spreads the peak scores over about 0.2..0.8 and makes
    the boxes about 32 px wide so that they overlap."""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, x):
        y = self.net(x).float()  # (B, S, 2+4, h, w)
        hm, off, wh = y.split([2, 2, 2], dim=2)
        hm = ((hm - hm.mean()) / hm.std() - 1.5) * 4.0
        return torch.cat([hm, off, wh + 8.0], dim=2)


def _tiny_prediction(nms, seed=PRED_SEED):
    from real_time_helmet_detection_amd.engine.evaluator import Prediction
    from real_time_helmet_detection_amd.models import StackedHourglass
    torch.manual_seed(seed)
    net = StackedHourglass(1, 32, 6).cuda().to(memory_format=CL).eval()
    pred = Prediction(SpreadHeads(net), topk=PRED_TOPK, scale_factor=4,
                      conf_th=PRED_CONF, nms=nms, nms_th=0.5).cuda()
    x = torch.randn(2, 3, 128, 128, device='cuda').contiguous(
        memory_format=CL)
    return pred, x


def _decoded_and_output(pred, x, monkeypatch):
    """Run pred(x), also returning the decoded candidates of that very
    forward as CPU tensors (boxes (2,N,4), clss (2,N), scores (2,N))."""
    decoded = {}
    real_decode = ops.batched_decode

    def recording_decode(*args, **kwargs):
        decoded['out'] = real_decode(*args, **kwargs)
        return decoded['out']

    monkeypatch.setattr(ops, 'batched_decode', recording_decode)
    with torch.no_grad():
        out = pred(x)
    monkeypatch.setattr(ops, 'batched_decode', real_decode)
    boxes, clss, scores = decoded['out']
    return (out, boxes.reshape(2, -1, 4).cpu(), clss.reshape(2, -1).cpu(),
            scores.reshape(2, -1).cpu())


def test_prediction_soft_nms_matches_eager_postprocessing(monkeypatch):
    pred, x = _tiny_prediction('soft-nms')
    # eager soft-NMS on the CPU over the decoded boxes of this very forward
    (box_lst, cls_lst, score_lst), boxes, clss, scores = \
        _decoded_and_output(pred, x, monkeypatch)
    assert len(box_lst) == 2 and scores.shape[1] == PRED_TOPK
    skipped = 0
    for i in range(2):
        _, _, ma, mb = case_margins(boxes[i], scores[i], PRED_CONF,
                                    score_th=PRED_CONF)
        print('image %d margins %.3g %.3g' % (i, ma, mb))
        if ma < MARGIN or mb < MARGIN:
            skipped += 1
            continue
        sel = (scores[i] >= PRED_CONF).nonzero().squeeze(1)
        keep, rescored = eager.soft_nms(boxes[i][sel], scores[i][sel],
                                        score_th=PRED_CONF)
        assert box_lst[i].shape[0] == keep.numel() > 0
        assert torch.equal(box_lst[i].cpu(), boxes[i][sel][keep])
        assert torch.equal(cls_lst[i].cpu(), clss[i][sel][keep])
        torch.testing.assert_close(score_lst[i].cpu(), rescored, rtol=RTOL,
                                   atol=0)
    assert skipped <= 1


def test_prediction_hard_nms_unchanged_by_the_shared_helper():
    pred, x = _tiny_prediction('nms')
    with torch.no_grad():
        box_lst, cls_lst, score_lst = pred(x)
    assert len(box_lst) == len(cls_lst) == len(score_lst) == 2
    for bx, sc in zip(box_lst, score_lst):
        assert bx.shape[0] == sc.shape[0] > 0
        assert (sc[:-1] >= sc[1:]).all()  # kept in descending-score order


def test_native_export_records_the_soft_nms_op():
    from real_time_helmet_detection_amd.engine.exporter import Export
    from real_time_helmet_detection_amd.models import StackedHourglass
    assert os.environ.get('RTHD_EAGER_GPU', '0') != '1'
    torch.manual_seed(7)
    net = StackedHourglass(1, 32, 6).cuda().to(memory_format=CL).eval()
    ex = Export(net, topk=50, scale_factor=4, conf_th=0.05, nms_th=0.5,
                nms='soft-nms').cuda().eval()
    x = torch.randn(1, 3, 128, 128, device='cuda')
    with torch.no_grad():
        want = ex(x)  # also warms the conv inference caches
        traced = torch.jit.trace(ex, x)
        got = traced(x)
    assert 'rthd::soft_nms' in str(traced.graph)
    assert want[0].shape[0] > 0
    for w, g in zip(want, got):
        torch.testing.assert_close(w, g)
