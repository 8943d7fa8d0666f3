"""Soft-NMS on the CPU: the batched eager twin, a float64 simulator of the
semantics, the scripted export variant and Export(nms='soft-nms').

The input generator and the simulator here are shared with
tests/test_gpu_soft_nms.py (the kernel's parity cases).
"""

import functools

import numpy as np
import pytest
import torch

from real_time_helmet_detection_amd.ops import eager
from real_time_helmet_detection_amd import ops

SIGMA = 0.5
SCORE_TH = 0.1   # Prediction passes conf_th for both thresholds
MARGIN = 1e-4    # a parity case is valid only above this (both margins)
PARITY_N = (63, 64, 65, 200, 256)


def clustered_boxes(n, seed):
    """n boxes around 8 cluster centres in a 512^2 frame: centre + N(0,10),
    sides 40-80 px, scores U(0.05, 1). Seeded, float32, CPU."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.rand(8, 2, generator=g) * 512
    which = torch.randint(0, 8, (n,), generator=g)
    c = centres[which] + torch.randn(n, 2, generator=g) * 10
    wh = 40 + 40 * torch.rand(n, 2, generator=g)
    boxes = torch.cat([c - wh / 2, c + wh / 2], dim=1)
    scores = 0.05 + 0.95 * torch.rand(n, generator=g)
    return boxes, scores


def simulate(boxes, scores, sigma, score_th):
    """Float64 numpy simulator of Gaussian soft-NMS over ALL given
    candidates. Returns (keep, kept_scores, margin_a, margin_b):
    margin_a = smallest relative gap between a round's winner and its
    runner-up, margin_b = smallest relative distance of any decayed score
    from score_th."""
    b = np.asarray(boxes, dtype=np.float64)
    s = np.asarray(scores, dtype=np.float64).copy()
    area = np.clip(b[:, 2] - b[:, 0], 0, None) * \
        np.clip(b[:, 3] - b[:, 1], 0, None)
    idx = np.arange(b.shape[0])
    keep, kept = [], []
    margin_a = margin_b = np.inf
    while idx.size:
        live = s[idx]
        top = int(np.argmax(live))          # first occurrence
        cur = idx[top]
        if idx.size > 1:
            second = np.max(np.delete(live, top))
            margin_a = min(margin_a,
                           abs(live[top] - second) / abs(live[top]))
        keep.append(int(cur))
        kept.append(float(s[cur]))
        rest = np.delete(idx, top)
        if rest.size == 0:
            break
        lt = np.maximum(b[cur, :2], b[rest, :2])
        rb = np.minimum(b[cur, 2:], b[rest, 2:])
        wh = np.clip(rb - lt, 0, None)
        inter = wh[:, 0] * wh[:, 1]
        union = np.clip(area[cur] + area[rest] - inter, 1e-9, None)
        iou = inter / union
        s[rest] = s[rest] * np.exp(-(iou * iou) / sigma)
        margin_b = min(margin_b,
                       float(np.min(np.abs(s[rest] - score_th))
                             / abs(score_th)))
        idx = rest[s[rest] > score_th]
    return keep, kept, margin_a, margin_b


def case_margins(boxes, scores, conf_th, sigma=SIGMA, score_th=SCORE_TH):
    """Simulate the candidates with score >= conf_th; indices are mapped
    back to the unfiltered numbering."""
    sel = (scores >= conf_th).nonzero(as_tuple=False).squeeze(1)
    if sel.numel() == 0:
        return [], [], np.inf, np.inf
    keep, kept, ma, mb = simulate(boxes[sel].numpy(), scores[sel].numpy(),
                                  sigma, score_th)
    return [int(sel[k]) for k in keep], kept, ma, mb


def first_valid(make, conf_th, what):
    """make(seed) -> (boxes, scores). First seed in 0..7 whose run keeps
    both margins >= MARGIN. Not finding one is a failure, never a skip."""
    for seed in range(8):
        boxes, scores = make(seed)
        keep, kept, ma, mb = case_margins(boxes, scores, conf_th)
        if ma >= MARGIN and mb >= MARGIN:
            return boxes, scores, keep, kept, seed
    pytest.fail('no seed in 0..7 gives margins >= %g for %s'
                % (MARGIN, what))


@functools.lru_cache(maxsize=None)
def parity_case(n, conf_th=SCORE_TH):
    return first_valid(lambda seed: clustered_boxes(n, seed), conf_th,
                       'N=%d' % n)


def batch_case(n=65):
    """B=3 with a different live count per image; image 2 has no candidate
    at or above conf_th. conf_th is 0.3."""
    conf_th = 0.3
    for seed in range(8):
        b0, s0 = clustered_boxes(n, seed)
        b1, s1 = clustered_boxes(n, seed + 100)
        b2, s2 = clustered_boxes(n, seed + 200)
        boxes = torch.stack([b0, b1, b2])
        scores = torch.stack([s0, s1 * 0.6, s2 * 0.25])
        ok = True
        for i in range(3):
            _, _, ma, mb = case_margins(boxes[i], scores[i], conf_th,
                                        score_th=conf_th)
            ok = ok and ma >= MARGIN and mb >= MARGIN
        if ok:
            return boxes, scores, conf_th
    pytest.fail('no seed in 0..7 gives a valid B=3 case')


def per_image_oracle(boxes, scores, sigma, score_th, conf_th):
    """eager.soft_nms per image on the candidates >= conf_th, i.e. what
    Prediction.forward did before the batched op existed."""
    out = []
    for i in range(boxes.shape[0]):
        sel = (scores[i] >= conf_th).nonzero(as_tuple=False).squeeze(1)
        keep, rescored = eager.soft_nms(boxes[i][sel], scores[i][sel],
                                        sigma=sigma, score_th=score_th)
        out.append((sel[keep], rescored))
    return out


def check_batched(got, want, rtol):
    """got = (idx, scores, counts) of a batched op, want = per_image_oracle
    output. Indices and counts exact, scores to rtol, tails zero. Returns
    the worst relative score error."""
    idx, sc, counts = (t.cpu() for t in got)
    assert idx.dtype == torch.int32 and counts.dtype == torch.int32
    assert sc.dtype == torch.float32
    worst = 0.0
    for i, (keep, rescored) in enumerate(want):
        k = int(counts[i])
        assert k == keep.numel(), (i, k, keep.numel())
        assert idx[i, :k].tolist() == keep.tolist()
        if k:
            rel = ((sc[i, :k] - rescored).abs() / rescored.abs()).max().item()
            worst = max(worst, rel)
        torch.testing.assert_close(sc[i, :k], rescored, rtol=rtol, atol=0)
        assert not idx[i, k:].any() and not sc[i, k:].any()
    return worst


# ------------------------------------------------------------------ tests --

def test_batched_eager_equals_per_image():
    boxes, scores, conf_th = batch_case()
    got = eager.soft_nms_batched(boxes, scores, SIGMA, conf_th, conf_th)
    want = per_image_oracle(boxes, scores, SIGMA, conf_th, conf_th)
    counts = got[2].tolist()
    assert counts[2] == 0 and len(set(counts)) == 3, counts
    assert got[0].shape == scores.shape and got[1].shape == scores.shape
    check_batched(got, want, rtol=0)


def test_dispatch_uses_eager_on_cpu():
    boxes, scores, conf_th = batch_case()
    got = ops.soft_nms_batched(boxes, scores, SIGMA, conf_th, conf_th)
    want = eager.soft_nms_batched(boxes, scores, SIGMA, conf_th, conf_th)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize('n', PARITY_N)
def test_eager_equals_simulator(n):
    """fp32 eager against the float64 simulator on margin-valid cases:
    same selection order; scores to 5e-6 relative (a few fp32 ulp of
    6e-8 per overlapping round from exp and the IoU quotient, about ten
    overlapping rounds per cluster, with a 5x allowance)."""
    boxes, scores, keep, kept, _ = parity_case(n)
    sel = (scores >= SCORE_TH).nonzero(as_tuple=False).squeeze(1)
    got_keep, got_sc = eager.soft_nms(boxes[sel], scores[sel], sigma=SIGMA,
                                      score_th=SCORE_TH)
    assert sel[got_keep].tolist() == keep
    np.testing.assert_allclose(got_sc.numpy().astype(np.float64),
                               np.asarray(kept), rtol=5e-6, atol=0)


def test_simulator_flags_ties():
    # two identical candidates: winner/runner-up gap 0 -> case not valid
    boxes = torch.tensor([[0., 0., 10., 10.], [20., 20., 30., 30.]])
    _, _, ma, _ = simulate(boxes.numpy(), np.array([0.5, 0.5]), SIGMA, 0.1)
    assert ma == 0.0


@pytest.mark.parametrize('n', (1, 2, 65, 200))
def test_scripted_equals_eager(n):
    from real_time_helmet_detection_amd.engine.exporter import \
        soft_nms_scripted
    boxes, scores = clustered_boxes(n, 3)
    want_keep, want_sc = eager.soft_nms(boxes, scores, sigma=SIGMA,
                                        score_th=SCORE_TH)
    keep, sc = soft_nms_scripted(boxes, scores, SIGMA, SCORE_TH)
    assert keep.dtype == torch.long
    assert keep.tolist() == want_keep.tolist()
    torch.testing.assert_close(sc, want_sc, rtol=1e-6, atol=0)


def test_scripted_empty():
    from real_time_helmet_detection_amd.engine.exporter import \
        soft_nms_scripted
    keep, sc = soft_nms_scripted(torch.zeros(0, 4), torch.zeros(0), SIGMA,
                                 SCORE_TH)
    assert keep.numel() == 0 and sc.numel() == 0


def test_export_soft_nms_traces_on_cpu():
    from real_time_helmet_detection_amd.models import StackedHourglass
    from real_time_helmet_detection_amd.engine.exporter import Export
    torch.manual_seed(0)
    net = StackedHourglass(num_stack=1, in_ch=16, out_ch=6).eval()
    ex = Export(net, topk=10, scale_factor=4, conf_th=0.0, nms_th=0.5,
                num_cls=2, nms='soft-nms').eval()
    x = torch.randn(1, 3, 64, 64)
    with torch.no_grad():
        want = ex(x)
        traced = torch.jit.trace(ex, x)
        y = torch.randn(1, 3, 64, 64)
        want_y = ex(y)
        got_y = traced(y)
        got = traced(x)
    assert want[0].dim() == 2 and want[0].shape[1] == 4
    assert want[0].shape[0] > 0
    for a, b in zip(want, got):
        torch.testing.assert_close(a, b)
    for a, b in zip(want_y, got_y):
        torch.testing.assert_close(a, b)


def test_export_default_is_hard_nms_and_args_pass_through():
    from real_time_helmet_detection_amd.config import build_parser
    from real_time_helmet_detection_amd.models import StackedHourglass
    from real_time_helmet_detection_amd.engine.exporter import (
        Export, build_export_module)
    net = StackedHourglass(num_stack=1, in_ch=16, out_ch=6).eval()
    assert Export(net, topk=10, scale_factor=4, conf_th=0.0,
                  nms_th=0.5).nms == 'nms'
    args = build_parser(['--num-stack', '1', '--hourglass-inch', '16',
                         '--nms', 'soft-nms'])
    assert build_export_module(args, net).nms == 'soft-nms'


def test_export_unknown_mode_raises():
    from real_time_helmet_detection_amd.models import StackedHourglass
    from real_time_helmet_detection_amd.engine.exporter import Export
    net = StackedHourglass(num_stack=1, in_ch=16, out_ch=6).eval()
    with pytest.raises(NotImplementedError):
        Export(net, topk=10, scale_factor=4, conf_th=0.0, nms_th=0.5,
               nms='bogus')
