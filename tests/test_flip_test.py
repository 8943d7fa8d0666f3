"""Flip testing on the CPU: the eager oracle ops.eager.decode_logits against
a per-pixel hand computation, the mirror identity, Prediction / Export with
flip_test, and the --flip-test flag end to end."""

import os
import subprocess
import sys

import pytest
import torch

from real_time_helmet_detection_amd import ops
from real_time_helmet_detection_amd.ops import eager

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sig(z):
    return torch.sigmoid(z)


def hand_decode(out, scale_factor, topk, pool_size, normalized):
    """decode_logits(flip=True) written out pixel by pixel, S == 1:
    merged maps from the definitions, peak test with > over the window,
    order score descending then index ascending, box arithmetic."""
    bt, s, k, h, w = out.shape
    assert s == 1
    b, c, r = bt // 2, k - 4, pool_size // 2
    sf = torch.tensor(float(scale_factor))
    rows = []
    for i in range(b):
        plain, mirr = out[i, 0].float(), out[b + i, 0].float()
        hm = torch.zeros(c, h, w)
        wh = torch.zeros(2, h, w)
        off = torch.zeros(2, h, w)
        for y in range(h):
            for x in range(w):
                for ch in range(c):
                    hm[ch, y, x] = 0.5 * (sig(plain[ch, y, x])
                                          + sig(mirr[ch, y, w - 1 - x]))
                for d in range(2):
                    a, m = plain[c + 2 + d, y, x], mirr[c + 2 + d, y,
                                                       w - 1 - x]
                    o = plain[c + d, y, x]
                    if normalized:
                        a, m, o = sig(a), sig(m), sig(o)
                    wh[d, y, x] = 0.5 * (a + m)
                    off[d, y, x] = o
        peaks = []
        for ch in range(c):
            for y in range(h):
                for x in range(w):
                    v = hm[ch, y, x]
                    win = hm[ch, max(0, y - r):y + r + 1,
                             max(0, x - r):x + r + 1]
                    if not bool((win > v).any()):
                        peaks.append((-float(v), (ch * h + y) * w + x))
        peaks.sort()
        img = []
        for negv, idx in peaks[:topk]:
            ch, rem = divmod(idx, h * w)
            y, x = divmod(rem, w)
            xo, yo, xs, ys = off[0, y, x], off[1, y, x], wh[0, y, x], \
                wh[1, y, x]
            if normalized:
                xo, yo, xs, ys = xo * sf, yo * sf, xs * w, ys * h
            xc, yc = x + xo, y + yo
            img.append(([float((xc - xs / 2) * sf), float((yc - ys / 2) * sf),
                         float((xc + xs / 2) * sf),
                         float((yc + ys / 2) * sf)], ch, hm[ch, y, x].item()))
        rows.append(img)
    boxes = torch.tensor([[r_[0] for r_ in img] for img in rows])
    clss = torch.tensor([[r_[1] for r_ in img] for img in rows])
    scores = torch.tensor([[r_[2] for r_ in img] for img in rows])
    return boxes, clss, scores


@pytest.mark.parametrize('normalized', (False, True))
def test_oracle_matches_hand_computation(normalized):
    torch.manual_seed(3)
    out = torch.randn(2, 1, 6, 8, 8) * 2
    want = hand_decode(out, 4, 6, 3, normalized)
    got = eager.decode_logits(out, 4, 6, 3, normalized, flip=True)
    assert got[0].shape == (1, 6, 4) and got[1].shape == (1, 6)
    assert got[1].dtype == torch.long
    assert torch.equal(got[2], want[2])
    assert torch.equal(got[1], want[1])
    torch.testing.assert_close(got[0], want[0], rtol=1e-6, atol=1e-5)


def mirror_pair(a, num_cls):
    """cat[a, mirror of a] with the mirrored half's offset channels
    overwritten by garbage: they must not be read."""
    m = a.flip(-1).clone()
    m[:, :, num_cls:num_cls + 2] = 1e4 * torch.randn_like(
        m[:, :, num_cls:num_cls + 2])
    return torch.cat([a, m])


@pytest.mark.parametrize('normalized', (False, True))
def test_mirror_identity(normalized):
    # 0.5f * (p + p) == p: merging an image's output with its own mirror
    # image changes nothing, bit for bit
    torch.manual_seed(4)
    a = torch.randn(2, 2, 6, 9, 11) * 2  # two different images
    want = ops.decode_logits(a, 4, 12, 3, normalized, flip=False)
    got = ops.decode_logits(mirror_pair(a, 2), 4, 12, 3, normalized,
                            flip=True)
    for w, g in zip(want, got):
        assert torch.equal(w, g)


def test_flip_off_is_the_present_composition():
    torch.manual_seed(5)
    out = torch.randn(3, 2, 6, 8, 8)
    flat = out.reshape(6, 6, 8, 8)
    hm, off, wh = flat.split([2, 2, 2], dim=1)
    want = eager.batched_decode(torch.sigmoid(hm), off, wh, 4, 5, 3, False)
    got = ops.decode_logits(out, 4, 5, 3, False)
    for w, g in zip(want, got):
        assert torch.equal(w, g)


def test_odd_batch_with_flip_raises():
    with pytest.raises((ValueError, RuntimeError)):
        ops.decode_logits(torch.randn(3, 1, 6, 8, 8), 4, 5, 3, False,
                          flip=True)


def tiny_net(seed=0):
    from real_time_helmet_detection_amd.models import StackedHourglass
    torch.manual_seed(seed)
    return StackedHourglass(num_stack=2, in_ch=16, out_ch=6).eval()


def test_prediction_flip_test_on_cpu():
    from real_time_helmet_detection_amd.engine.evaluator import Prediction
    net = tiny_net()
    topk = 10
    pred = Prediction(net, topk=topk, scale_factor=4, conf_th=0.0,
                      nms='nms', nms_th=0.5, flip_test=True).eval()
    assert not Prediction(net, topk=topk, scale_factor=4, conf_th=0.0,
                          nms='nms', nms_th=0.5).flip_test
    x = torch.randn(2, 3, 64, 64)
    with torch.no_grad():
        box_lst, cls_lst, score_lst = pred(x)
        # the same by hand around the same network
        out = net(torch.cat([x, x.flip(3)])).float()
        plain, mirr = out[:2], out[2:].flip(-1)
        hm = 0.5 * (torch.sigmoid(plain[:, :, :2])
                    + torch.sigmoid(mirr[:, :, :2]))
        wh = 0.5 * (plain[:, :, 4:] + mirr[:, :, 4:])
        off = plain[:, :, 2:4]
        h, w = hm.shape[-2:]
        boxes, clss, scores = eager.batched_decode(
            hm.reshape(4, 2, h, w), off.reshape(4, 2, h, w),
            wh.reshape(4, 2, h, w), 4, topk, 3, False)
    boxes = boxes.reshape(2, 2 * topk, 4)
    clss = clss.reshape(2, 2 * topk)
    scores = scores.reshape(2, 2 * topk)
    assert len(box_lst) == 2
    for i in range(2):
        keep = eager.nms(boxes[i], scores[i], 0.5)
        assert keep.numel() > 0
        assert torch.equal(box_lst[i], boxes[i][keep])
        assert torch.equal(cls_lst[i], clss[i][keep])
        assert torch.equal(score_lst[i], scores[i][keep])


def test_export_flip_test_traces_on_cpu():
    from real_time_helmet_detection_amd.engine.exporter import Export
    net = tiny_net(1)
    ex = Export(net, topk=10, scale_factor=4, conf_th=0.0, nms_th=0.5,
                num_cls=2, flip_test=True).eval()
    plain = Export(net, topk=10, scale_factor=4, conf_th=0.0, nms_th=0.5,
                   num_cls=2).eval()
    assert not plain.flip_test
    x = torch.randn(1, 3, 64, 64)
    with torch.no_grad():
        want = ex(x)
        traced = torch.jit.trace(ex, x)
        y = torch.randn(1, 3, 64, 64)
        want_y = ex(y)
        got_y = traced(y)
        got = traced(x)
        unflipped = plain(x)
    assert want[0].dim() == 2 and want[0].shape[1] == 4
    assert want[0].shape[0] > 0
    for a, b in zip(want, got):
        torch.testing.assert_close(a, b)
    for a, b in zip(want_y, got_y):
        torch.testing.assert_close(a, b)
    # and the mirror pass does take part
    assert want[2].shape != unflipped[2].shape or \
        not torch.equal(want[2], unflipped[2])


def test_flag_parses_and_reaches_the_export_module():
    from real_time_helmet_detection_amd.config import (build_parser,
                                                       ARCH_FLAGS)
    from real_time_helmet_detection_amd.engine.exporter import \
        build_export_module
    net = tiny_net()
    base = ['--num-stack', '2', '--hourglass-inch', '16']
    off = build_parser(base)
    on = build_parser(base + ['--flip-test'])
    assert off.flip_test is False and on.flip_test is True
    assert 'flip_test' not in ARCH_FLAGS
    assert build_export_module(off, net).flip_test is False
    assert build_export_module(on, net).flip_test is True


def test_main_eval_cli_with_flip_test(tmp_path):
    """main.py evaluation on synthetic CPU data with --flip-test writes the
    prediction files, and the flag is recorded with the run."""
    save = str(tmp_path / 'run')
    env = dict(os.environ)
    env['PYTHONPATH'] = REPO
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, 'main.py'),
         '--synthetic', '--synthetic-size', '2', '--gpu-no', '-1',
         '--num-workers', '0', '--imsize', '64', '--batch-size', '2',
         '--num-stack', '1', '--hourglass-inch', '16', '--topk', '10',
         '--save-path', save, '--flip-test'],
        cwd=str(tmp_path), env=env, capture_output=True, text=True,
        timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert os.path.isfile(os.path.join(save, 'prediction_results.pickle'))
    assert os.path.isdir(os.path.join(save, 'txt')), os.listdir(save)
    with open(os.path.join(save, 'argument.txt')) as f:
        assert 'flip_test: True' in f.read()
