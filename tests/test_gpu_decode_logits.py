"""The logits-in decode kernel (ops/csrc/decode.hip, decode_logits) against
the CPU oracle ops.eager.decode_logits, and flip testing through
Prediction, GraphedPredictor and the native export.

Tolerances are those of test_decode_matches_eager: scores rtol 1e-5 / atol
1e-6, boxes 1e-4, classes exact, compared after sorting by score.

CPU and device expf differ in the last ulp, so the parity inputs make the
comparison independent of that: heatmap logits come from a coarse grid of
multiples of 1/8 (exact in bf16) on which different scores are far apart.
- flip off: the 73 multiples of 1/8 in [-6, 3]; two different p(z) are at
  least 3.2e-4 apart.
- flip on: the 12 values -5.875 + 0.75 k. z in this grid never has -z in it,
  so the p(z) + p(-z) = 1 family (equal in exact arithmetic, an ulp apart in
  fp32) does not occur, and over the WHOLE grid two different merged scores
  0.5 (p(a) + p(b)) are at least 4.3e-4 apart (float64 enumeration).
oracle_ok asserts the 1e-4 of the input condition on every peak candidate
of the CPU oracle. Exact ties are plentiful (local maxima crowd the top of
the grid); rows of equal score are compared as a set, and topk either
exceeds the number of peaks or ends exactly behind the planted peaks, so it
never cuts through a tie group, where torch.topk may pick any member
(oracle_ok asserts that too). Selection of topk among continuous scores is
covered by the Prediction case.
"""

import functools
import os

import pytest
import torch

from real_time_helmet_detection_amd import ops
from real_time_helmet_detection_amd.ops import eager

pytestmark = pytest.mark.gpu

CL = torch.channels_last
TW, TH = 32, 8  # scan tile of decode_logits (decode.hip)
# heatmap logit grids: (background values, weak and strong planted peak)
COARSE = -5.875 + 0.75 * torch.arange(12, dtype=torch.float32)
FINE = -6.0 + 0.125 * torch.arange(73, dtype=torch.float32)
GRIDS = {True: (COARSE[:10], COARSE[10], COARSE[11]),   # flip on
         False: (FINE[:65], FINE[68], FINE[72])}        # flip off
GAP = 1e-4


def plant(hm, b_plain, b_mirr, s, c, y, x, val):
    """Put a heatmap logit at merged position (y, x): in the plain half and,
    under flip, at the mirrored column of the mirrored half."""
    w = hm.shape[-1]
    hm[b_plain, s, c, y, x] = val
    if b_mirr is not None:
        hm[b_mirr, s, c, y, w - 1 - x] = val


def make_logits(bt, s, c, h, w, flip, normalized, seed):
    """(bt, s, c+4, h, w) fp32 logits, every value exact in bf16."""
    g = torch.Generator().manual_seed(seed)
    back, WEAK, STRONG = GRIDS[flip]
    hm = back[torch.randint(0, len(back), (bt, s, c, h, w), generator=g)]
    if normalized:
        geom = torch.randint(-24, 25, (bt, s, 4, h, w), generator=g) / 8.0
    else:
        off = torch.randint(0, 8, (bt, s, 2, h, w), generator=g) / 8.0
        wh = torch.randint(4, 81, (bt, s, 2, h, w), generator=g) / 4.0
        geom = torch.cat([off, wh], dim=2)
    b = bt // 2 if flip else bt
    xseams = list(range(TW, w, TW))
    yseams = list(range(TH, h, TH))
    for i in range(b):
        m = b + i if flip else None
        for st in range(s):
            cls = (i + st) % c
            put = functools.partial(plant, hm, i, m, st, cls)
            # map corners and edges
            put(0, 0, STRONG)
            put(0, w - 1, STRONG)
            put(h - 1, 0, STRONG)
            put(h - 1, w - 1, STRONG)
            put(h // 2, 0, WEAK)
            put(h // 2, w - 1, WEAK)
            put(0, w // 2 - 3, WEAK)
            put(h - 1, w // 2 + 3, WEAK)
            # both sides of every tile seam, once with the stronger value
            # on each side: the weaker one is a peak only if the halo (or
            # the mirrored column) is off by one
            for xs in xseams:
                put(3, xs - 1, STRONG)
                put(3, xs, WEAK)
                put(h - 4, xs - 1, WEAK)
                put(h - 4, xs, STRONG)
            for ys in yseams:
                put(ys - 1, 5, STRONG)
                put(ys, 5, WEAK)
                put(ys - 1, w - 6, WEAK)
                put(ys, w - 6, STRONG)
    return torch.cat([hm, geom], dim=2)


# name -> bt, s, c, h, w, pool, topk, normalized. seams_p3 and the odd cases
# list every peak and then zero-score rows; seams_p5 lists exactly the 14
# planted peaks that survive (all above every background score)
SHAPES = {
    'seams_p3': (4, 2, 2, 24, 40, 3, 300, False),
    'seams_p5': (4, 2, 2, 24, 40, 5, 14, False),
    'odd_p7': (2, 1, 3, 17, 19, 7, 100, False),
    'odd_p7_norm': (2, 1, 3, 17, 19, 7, 100, True),
}
SEED = 0  # oracle_ok holds for every case at this seed


def oracle_ok(out, pool, topk, normalized, flip):
    """The input condition, on the CPU oracle alone: among ALL its peak
    candidates two different scores are more than GAP apart, and topk does
    not cut through a group of equal scores. Returns (ok, why)."""
    n = (out.shape[2] - 4) * out.shape[3] * out.shape[4]
    _, _, s_all = eager.decode_logits(out, 4, n, pool, normalized, flip)
    s_all = s_all.sort(dim=1, descending=True).values
    for i in range(s_all.shape[0]):
        s = s_all[i][s_all[i] > 0]
        d = s[:-1] - s[1:]
        if bool(((d > 0) & (d <= GAP)).any()):
            return False, 'image %d: scores closer than %g' % (i, GAP)
        if topk < s.numel() and s[topk - 1] == s[topk]:
            return False, 'image %d: topk cuts a tie group' % i
    return True, ''


@functools.lru_cache(maxsize=None)
def parity_case(name, flip):
    bt, s, c, h, w, pool, topk, normalized = SHAPES[name]
    out = make_logits(bt, s, c, h, w, flip, normalized, SEED)
    ok, why = oracle_ok(out, pool, topk, normalized, flip)
    assert ok, why
    want = eager.decode_logits(out, 4, topk, pool, normalized, flip)
    return out, want


def check_rows(got, want):
    """got (device) against want (oracle): scores after sorting, then per
    group of equal oracle score the (class, box) rows as a set. Returns the
    worst relative score error."""
    gb, gc, gs = (t.cpu() for t in got)
    wb, wc, ws = want
    assert gb.shape == wb.shape and gc.shape == wc.shape
    assert gc.dtype == torch.long and gs.dtype == torch.float32
    worst = 0.0
    for i in range(ws.shape[0]):
        w_s, wo = ws[i].sort(descending=True, stable=True)
        g_s, go = gs[i].sort(descending=True, stable=True)
        torch.testing.assert_close(g_s, w_s, rtol=1e-5, atol=1e-6)
        live = w_s > 0
        if live.any():
            worst = max(worst, ((g_s - w_s).abs()[live] / w_s[live]).max()
                        .item())
        # zero-score rows sit at index 0
        assert not gs[i][go][~live].any()
        assert not gc[i][go][~live].any()
        k = int(live.sum())
        j = 0
        while j < k:
            e = j
            while e < k and w_s[e] == w_s[j]:
                e += 1
            free = list(range(j, e))
            for r in range(j, e):
                hit = None
                for q in free:
                    if wc[i][wo[r]] == gc[i][go[q]] and torch.allclose(
                            wb[i][wo[r]], gb[i][go[q]], rtol=1e-4,
                            atol=1e-4):
                        hit = q
                        break
                assert hit is not None, (i, r, wb[i][wo[r]], wc[i][wo[r]])
                free.remove(hit)
            j = e
    return worst


@pytest.mark.parametrize('dtype', (torch.float32, torch.bfloat16),
                         ids=('fp32', 'bf16'))
@pytest.mark.parametrize('flip', (False, True), ids=('plain', 'flip'))
@pytest.mark.parametrize('name', sorted(SHAPES))
def test_kernel_matches_oracle(name, flip, dtype):
    out, want = parity_case(name, flip)
    _, _, _, _, _, pool, topk, normalized = SHAPES[name]
    lo = out.to(dtype)
    assert torch.equal(lo.float(), out)  # exact in bf16
    got = ops.decode_logits(lo.cuda(), 4, topk, pool, normalized, flip)
    assert all(t.is_cuda for t in got)
    if name.startswith('odd'):
        assert (want[2] == 0).any()  # topk exceeds the number of peaks
    worst = check_rows(got, want)
    print('%s flip=%s %s worst relative score error %.3g'
          % (name, flip, dtype, worst))


def test_strided_input_is_made_dense():
    out, want = parity_case('seams_p3', True)
    wide = torch.zeros(out.shape[:-1] + (out.shape[-1] + 3,))
    wide[..., :out.shape[-1]] = out
    view = wide.cuda()[..., :out.shape[-1]]
    assert not view.is_contiguous()
    check_rows(ops.decode_logits(view, 4, 300, 3, False, True), want)


@pytest.mark.parametrize('dtype', (torch.float32, torch.bfloat16),
                         ids=('fp32', 'bf16'))
@pytest.mark.parametrize('normalized', (False, True))
def test_mirror_identity_is_bitwise(dtype, normalized):
    # 0.5f * (p + p) == p; two different images, so that a b / B+b mix-up
    # shows; the mirrored half's offsets are garbage and must not be read
    torch.manual_seed(11)
    a = (torch.randn(2, 2, 6, 17, 19) * 2).to(dtype)
    m = a.flip(-1).clone()
    m[:, :, 2:4] = (1e4 * torch.randn(2, 2, 2, 17, 19)).to(dtype)
    want = ops.decode_logits(a.cuda(), 4, 25, 3, normalized, False)
    got = ops.decode_logits(torch.cat([a, m]).cuda(), 4, 25, 3, normalized,
                            True)
    assert (want[2] > 0).all()
    for w, g in zip(want, got):
        assert torch.equal(w, g)


@pytest.mark.parametrize('dtype', (torch.float32, torch.bfloat16),
                         ids=('fp32', 'bf16'))
def test_overflow_path(dtype):
    """Every heatmap logit equal: all 9216 positions are peaks, more than
    the peak buffer holds, so the emit stage re-scans the logits. The
    winners are the lowest indices; torch.topk leaves ties open, so the
    expected rows come straight from the formulas."""
    c, h, w, topk = 2, 72, 64, 50
    g = torch.Generator().manual_seed(2)
    out = torch.empty(2, 1, c + 4, h, w)
    out[0, :, :c] = 0.625
    out[1, :, :c] = -0.125
    out[:, :, c:c + 2] = torch.randint(0, 8, (2, 1, 2, h, w),
                                       generator=g) / 8.0
    out[:, :, c + 2:] = torch.randint(4, 81, (2, 1, 2, h, w),
                                      generator=g) / 4.0
    boxes, clss, scores = ops.decode_logits(out.to(dtype).cuda(), 4, topk, 3,
                                            False, True)
    score = 0.5 * (torch.sigmoid(torch.tensor(0.625))
                   + torch.sigmoid(torch.tensor(-0.125)))
    torch.testing.assert_close(scores.cpu(), score.expand(1, topk),
                               rtol=1e-5, atol=1e-6)
    assert not clss.any()
    x = torch.arange(topk)  # index i is (class 0, y 0, x i)
    xo, yo = out[0, 0, c, 0, x], out[0, 0, c + 1, 0, x]
    xs = 0.5 * (out[0, 0, c + 2, 0, x] + out[1, 0, c + 2, 0, w - 1 - x])
    ys = 0.5 * (out[0, 0, c + 3, 0, x] + out[1, 0, c + 3, 0, w - 1 - x])
    xc, yc = x + xo, 0 + yo
    want = torch.stack([(xc - xs / 2) * 4, (yc - ys / 2) * 4,
                        (xc + xs / 2) * 4, (yc + ys / 2) * 4], dim=1)
    torch.testing.assert_close(boxes[0].cpu(), want, rtol=1e-4, atol=1e-4)


def test_wide_pool_runs_the_eager_composition():
    out, _ = parity_case('seams_p3', True)
    want = eager.decode_logits(out, 4, 8, 9, False, True)
    got = ops.decode_logits(out.cuda(), 4, 8, 9, False, True)
    assert got[0].is_cuda
    torch.testing.assert_close(got[2].cpu(), want[2], rtol=1e-5, atol=1e-6)


def test_odd_batch_with_flip_raises():
    with pytest.raises(RuntimeError, match='even batch'):
        ops.decode_logits(torch.zeros(3, 1, 6, 8, 8, device='cuda'), 4, 5, 3,
                          False, True)


def test_graph_capture_and_replay():
    out, want = parity_case('seams_p3', True)
    static = torch.zeros_like(out).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.decode_logits(static, 4, 300, 3, False, True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = ops.decode_logits(static, 4, 300, 3, False, True)
    for _ in range(2):  # the workspace is zeroed inside the graph
        static.copy_(out)
        graph.replay()
        torch.cuda.synchronize()
        check_rows(got, want)


# ------------------------------------------------------------ predictors ---

PRED_TOPK = 20
PRED_CONF = 0.05


class SpreadHeads(torch.nn.Module):
    """The tiny net with an affine map on its raw output (the idea of
    tests/test_gpu_soft_nms.py): an untrained net puts every peak score
    within 0.02 of the others; this spreads them over about 0.2..0.8 and
    makes the boxes wide enough to overlap."""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, x):
        y = self.net(x).float()  # (B, S, 2+4, h, w)
        hm, off, wh = y.split([2, 2, 2], dim=2)
        hm = ((hm - hm.mean()) / hm.std() - 1.5) * 4.0
        return torch.cat([hm, off, wh + 8.0], dim=2)


def tiny_net(seed):
    from real_time_helmet_detection_amd.models import StackedHourglass
    torch.manual_seed(seed)
    return StackedHourglass(1, 32, 6).cuda().to(memory_format=CL).eval()


def test_prediction_flip_test(monkeypatch):
    from real_time_helmet_detection_amd.engine.evaluator import Prediction
    pred = Prediction(SpreadHeads(tiny_net(0)), topk=PRED_TOPK,
                      scale_factor=4, conf_th=PRED_CONF, nms='nms',
                      nms_th=0.5, flip_test=True).cuda()
    x = torch.randn(2, 3, 64, 64, device='cuda').contiguous(memory_format=CL)
    seen = {}
    real = ops.decode_logits

    def recording(out, *args, **kwargs):
        seen['out'] = out
        seen['args'] = (args, kwargs)
        seen['res'] = real(out, *args, **kwargs)
        return seen['res']

    monkeypatch.setattr(ops, 'decode_logits', recording)
    with torch.no_grad():
        box_lst, cls_lst, score_lst = pred(x)
    monkeypatch.setattr(ops, 'decode_logits', real)

    out = seen['out']
    assert out.shape[0] == 4 and seen['args'][1] == {'flip': True}
    # candidates: the CPU oracle on this very forward's logits
    want = eager.decode_logits(out.cpu(), 4, PRED_TOPK, 3, False, flip=True)
    worst = check_rows(seen['res'], want)
    print('prediction worst relative score error %.3g' % worst)
    # final lists: eager NMS of those very candidates, exactly
    boxes, clss, scores = (t.cpu() for t in seen['res'])
    assert len(box_lst) == 2
    for i in range(2):
        sel = (scores[i] >= PRED_CONF).nonzero().squeeze(1)
        keep = eager.nms(boxes[i][sel], scores[i][sel], 0.5)
        assert keep.numel() > 0
        assert torch.equal(box_lst[i].cpu(), boxes[i][sel][keep])
        assert torch.equal(cls_lst[i].cpu(), clss[i][sel][keep])
        assert torch.equal(score_lst[i].cpu(), scores[i][sel][keep])


def test_graphed_predictor_flip_test_equals_ungraphed():
    from real_time_helmet_detection_amd import amp
    from real_time_helmet_detection_amd.engine.evaluator import (
        Prediction, GraphedPredictor)
    pred = Prediction(tiny_net(8), topk=PRED_TOPK, scale_factor=4,
                      conf_th=0.1, nms='nms', nms_th=0.5,
                      flip_test=True).cuda()
    xs = [torch.randn(2, 3, 64, 64, device='cuda').contiguous(
        memory_format=CL) for _ in range(2)]
    with torch.no_grad(), amp.autocast(True):
        wants = [pred(x) for x in xs]
    g = GraphedPredictor(pred, xs[0].clone())
    assert g.static_in.shape == xs[0].shape
    for x, want in zip(xs, wants):  # two inputs through one capture
        got = g(x)
        for wl, gl in zip(want, got):
            assert len(wl) == len(gl) == 2
            for wt, gt in zip(wl, gl):
                assert torch.equal(wt, gt)
    assert any(len(b) for b in wants[0][0])


def test_native_export_records_decode_logits():
    from real_time_helmet_detection_amd.engine.exporter import Export
    assert os.environ.get('RTHD_EAGER_GPU', '0') != '1'
    ex = Export(tiny_net(7), topk=50, scale_factor=4, conf_th=0.05,
                nms_th=0.5, flip_test=True).cuda().eval()
    x = torch.randn(1, 3, 128, 128, device='cuda')
    with torch.no_grad():
        want = ex(x)  # also warms the conv inference caches
        traced = torch.jit.trace(ex, x)
        got = traced(x)
    graph = str(traced.inlined_graph)
    assert 'rthd::decode_logits' in graph
    assert 'rthd::decode(' not in graph
    assert want[0].shape[0] > 0
    for w, g in zip(want, got):
        torch.testing.assert_close(w, g)
