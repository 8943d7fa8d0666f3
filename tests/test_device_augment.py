"""--device-augment on CPU: sample_params / transform_boxes reproduce
TrainAugmentor.__call__'s draws and boxes, the eager oracle
ops.eager.augment_images pins the resampling convention exactly and stays
close to the PIL chain, and the flag trains through main.py."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from real_time_helmet_detection_amd.config import ARCH_FLAGS, build_parser
from real_time_helmet_detection_amd.data import SyntheticVOC, TrainAugmentor
from real_time_helmet_detection_amd.data.augment import (AugParams,
                                                         map_coefficients,
                                                         transform_boxes)
from real_time_helmet_detection_amd.ops import eager
from real_time_helmet_detection_amd.ops import functional as opsF

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------- draw order ---

def _boxes_for(w, h):
    """Ordinary boxes, one that already pokes out of the canvas, and one
    near the corner that scale 1.5 / a translate pushes out entirely."""
    return (np.array([[0.1 * w, 0.2 * h, 0.5 * w, 0.7 * h],
                      [0.6 * w, 0.5 * h, 1.2 * w, 1.1 * h],
                      [0.0, 0.0, 0.06 * w, 0.06 * h],
                      [0.4 * w, 0.4 * h, 0.6 * w, 0.6 * h]], np.float32),
            np.array([0, 1, 1, 0]))


@pytest.mark.parametrize('multiscale_flag', [False, True])
@pytest.mark.parametrize('crop_percent', [(0.0, 0.1), (0.5, 0.6)])
def test_sample_params_reproduce_call(multiscale_flag, crop_percent):
    """Same seed -> same T, labels and boxes (1e-3 px; fp32 coordinates
    below 1024 carry about 6e-5) as TrainAugmentor.__call__, over batches of
    three differently sized images. crop_percent (0.5, 0.6) makes
    top + bottom >= h every time: the skipped crop."""
    sizes = [(512, 512), (500, 375), (96, 64)]
    rng = np.random.RandomState(0)
    imgs = [rng.randint(0, 256, (h, w, 3), dtype=np.uint8) for w, h in sizes]
    boxes, labels = zip(*[_boxes_for(w, h) for w, h in sizes])
    kw = dict(multiscale_flag=multiscale_flag, crop_percent=crop_percent,
              seed=21)
    a, b = TrainAugmentor(**kw), TrainAugmentor(**kw)
    dropped = skipped = 0
    targets = set()
    for _ in range(6):  # consecutive batches: the streams stay in step
        _, want_b, want_l = a(list(imgs), list(boxes), list(labels))
        params, T = b.sample_params(sizes)
        targets.add(T)
        assert len(params) == 3
        for i, (p, wh) in enumerate(zip(params, sizes)):
            got_b, got_l = transform_boxes(boxes[i], labels[i], p, wh, T)
            assert got_b.dtype == np.float32 and got_b.shape[1:] == (4,)
            assert got_l.tolist() == want_l[i].tolist()
            assert got_b.shape == want_b[i].shape
            if len(got_b):
                assert np.abs(got_b - want_b[i]).max() <= 1e-3
                assert got_b.min() >= 0 and got_b.max() <= T
            dropped += len(labels[i]) - len(got_l)
            skipped += (p.top, p.bottom, p.left, p.right) == (0, 0, 0, 0)
    assert dropped > 0, 'no box ever left the image'
    if crop_percent[0] >= 0.5:
        assert skipped == 18
    if multiscale_flag:
        assert targets <= {320, 384, 448} and len(targets) > 1
    else:
        assert targets == {512}


# ------------------------------------------------------ convention pins ---

def _oracle(img, coef, T, sizes=None):
    """eager.augment_images on a (B,H,W,3) uint8 array, uint8 out."""
    img = torch.as_tensor(img)
    if sizes is None:
        sizes = [[img.shape[1], img.shape[2]]] * img.shape[0]
    return eager.augment_images(
        img, torch.tensor(sizes, dtype=torch.int32),
        torch.tensor(coef, dtype=torch.float32), T)


def _noise(h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (1, h, w, 3), dtype=torch.uint8,
                         generator=g)


def test_identity_returns_input():
    img = _noise(24, 24)
    assert torch.equal(_oracle(img, [[1, 0, 1, 0, 1]], 24), img)


def test_pure_flip():
    img = _noise(24, 24)
    p = AugParams(1.0, 1.0, 0.0, 0.0, 0, 0, 0, 0, True)
    coef = list(map_coefficients(p, (24, 24), 24)) + [1.0]
    assert coef[:4] == [-1.0, 24.0, 1.0, 0.0]
    assert torch.equal(_oracle(img, [coef], 24), img.flip(2))


def test_integer_translate_is_shift_with_zero_fill():
    img = _noise(20, 28)
    # content moves right by 3 and up by 2: src = out - t
    p = AugParams(1.0, 1.0, 3.0, -2.0, 0, 0, 0, 0, False)
    ax, bx, ay, by = map_coefficients(p, (28, 20), 28)
    # T = w only; give y its own unit scale so the output is 28 x 28
    got = _oracle(img, [[ax, bx, 1.0, by, 1.0]], 28)
    want = torch.zeros(1, 28, 28, 3, dtype=torch.uint8)
    want[:, :18, 3:] = img[:, 2:, :25]
    assert bx == -3.0 and by == 2.0
    assert torch.equal(got, want)


def test_scale_two_is_rounded_two_tap_mean():
    img = _noise(16, 16)
    got = _oracle(img, [[2, 0, 2, 0, 1]], 8)
    f = img.float()
    # fx = fy = 0.5: top/bot are exact halves of sums, so is their mean
    top = f[:, 0::2, 0::2] * 0.5 + f[:, 0::2, 1::2] * 0.5
    bot = f[:, 1::2, 0::2] * 0.5 + f[:, 1::2, 1::2] * 0.5
    want = torch.floor(top * 0.5 + bot * 0.5 + 0.5).to(torch.uint8)
    assert torch.equal(got, want)
    # one axis only: the plain rounded mean of two neighbours
    got_x = _oracle(img, [[2, 0, 1, 0, 1]], 16)[:, :, :8]
    want_x = torch.floor((f[:, :, 0::2] + f[:, :, 1::2]) * 0.5 + 0.5)
    assert torch.equal(got_x, want_x.to(torch.uint8))


def test_brightness_truncates_and_saturates():
    vals = [0, 1, 3, 101, 169, 170, 171, 255]
    img = torch.tensor(vals, dtype=torch.uint8).view(1, 1, 8, 1)
    img = img.expand(1, 8, 8, 3).contiguous()
    got = _oracle(img, [[1, 0, 1, 0, 1.5]], 8)
    # 1.5: 1 -> 1 (1.5 truncated), 3 -> 4, 101 -> 151, 169 -> 253,
    # 170 -> 255 exactly, 171 and 255 saturate
    want = torch.tensor([0, 1, 4, 151, 253, 255, 255, 255],
                        dtype=torch.uint8)
    assert torch.equal(got[0, 3, :, 1], want)
    # the numpy arithmetic of multiply_brightness for a non-dyadic factor
    factor = 1.2345
    ramp = np.arange(256, dtype=np.uint8)
    want = np.clip(ramp.astype(np.float32) * factor, 0, 255).astype(np.uint8)
    img = torch.from_numpy(ramp).view(1, 16, 16, 1).expand(1, 16, 16, 3)
    got = _oracle(img.contiguous(), [[1, 0, 1, 0, factor]], 16)
    assert torch.equal(got[0, :, :, 2].reshape(-1), torch.from_numpy(want))


def test_padding_is_never_read():
    """An image smaller than its canvas: 255 in the padding changes
    nothing, for a map that looks well past the image on every side."""
    small = _noise(17, 23, seed=3)
    sizes = [[17, 23]]
    coef = [[1.7, -6.0, 1.3, -3.5, 1.25]]
    zero = torch.zeros(1, 30, 40, 3, dtype=torch.uint8)
    full = torch.full((1, 30, 40, 3), 255, dtype=torch.uint8)
    zero[:, :17, :23] = small
    full[:, :17, :23] = small
    a = _oracle(zero, coef, 32, sizes)
    b = _oracle(full, coef, 32, sizes)
    assert torch.equal(a, b)
    # and the same image without any canvas around it
    assert torch.equal(a, _oracle(small, coef, 32))
    assert a.any() and not a[:, -1].any()  # black beyond the image


def test_normalised_output_is_normalize_of_uint8():
    img = _noise(20, 20, seed=5)
    coef = [[0.8, 1.5, 1.1, -2.0, 1.3]]
    sizes = torch.tensor([[20, 20]], dtype=torch.int32)
    q = _oracle(img, coef, 12)
    for dtype in (torch.float32, torch.bfloat16):
        got = eager.augment_images(img, sizes, torch.tensor(coef), 12,
                                   'imagenet', dtype)
        assert got.shape == (1, 3, 12, 12) and got.dtype == dtype
        assert got.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(got, eager.normalize_images(q, 'imagenet', dtype))


# ------------------------------------------- closeness to the PIL chain ---

def _smooth_image(w, h):
    """Sums of sinusoids, every period >= 19 px, values within [1, 169]."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    chans = []
    for c, (px, py, pd) in enumerate([(19, 31, 47), (23, 41, 29),
                                      (37, 21, 53)]):
        chans.append(85 + 28 * np.sin(2 * np.pi * x / px + c)
                     + 28 * np.sin(2 * np.pi * y / py + 2 * c)
                     + 28 * np.sin(2 * np.pi * (x + y) / pd))
    img = np.stack(chans, -1)
    assert img.min() >= 0 and img.max() <= 170
    return img.astype(np.uint8)


# Mean |oracle - TrainAugmentor.__call__| in uint8 levels over seeds 0..19,
# measured with this oracle on this image:
#   (512, 512) -> 512: worst 0.704, mean 0.543
#   (500, 375) -> 320: worst 1.191, mean 0.836
# (a numpy sketch of the semantics on another smooth image gave worst 0.61,
# mean about 0.45). The bound is twice the worst of each case. What
# differs is rounding to uint8 once instead of three times, borders blurred
# three times against once, and at 320 the antialiased final resize of the
# PIL chain. A quarter-pixel error in the map costs about 2.4 on both
# cases; the wrong flip costs more than 13.
@pytest.mark.parametrize('size,target,bound', [
    ((512, 512), 512, 2 * 0.704), ((500, 375), 320, 2 * 1.191)])
def test_close_to_pil_chain(size, target, bound):
    w, h = size
    img = _smooth_image(w, h)
    img_t = torch.from_numpy(img)[None]
    sizes = torch.tensor([[h, w]], dtype=torch.int32)
    none = np.zeros((0, 4), np.float32), np.zeros((0,), np.int64)
    worst, total, worst_flipped = 0.0, 0.0, np.inf
    for seed in range(20):
        kw = dict(multiscale=(target, target, 64), seed=seed)
        want, _, _ = TrainAugmentor(**kw)([img], [none[0]], [none[1]])
        (p,), T = TrainAugmentor(**kw).sample_params([size])
        assert T == target and want[0].shape == (T, T, 3)

        def mad(params):
            coef = list(map_coefficients(params, size, T)) + [params.factor]
            got = eager.augment_images(
                img_t, sizes, torch.tensor([coef], dtype=torch.float64)
                .float(), T)
            return (got[0].numpy().astype(np.int32)
                    - want[0].astype(np.int32)).__abs__().mean()

        d = mad(p)
        worst, total = max(worst, d), total + d
        # negative control: the same draw with the flip bit inverted
        worst_flipped = min(worst_flipped, mad(p._replace(flip=not p.flip)))
    print('%s -> %d: worst %.3f mean %.3f, flipped min %.3f'
          % (size, target, worst, total / 20, worst_flipped))
    assert worst <= bound
    assert worst_flipped > bound


# ------------------------------------------------------ flag and parser ---

def test_flag_default_and_implication():
    off = build_parser([])
    assert off.device_augment is False and off.device_encode is False
    on = build_parser(['--device-augment'])
    assert on.device_augment is True and on.device_encode is True
    enc = build_parser(['--device-encode'])
    assert enc.device_encode is True and enc.device_augment is False
    assert 'device_augment' not in ARCH_FLAGS


def test_collate_device_aug_and_prepare_batch():
    from real_time_helmet_detection_amd.engine.trainer import prepare_batch

    class Mixed(SyntheticVOC):
        """Synthetic items cut to different sizes, one without boxes, one
        large enough to be integer-reduced (limit = 2 * 64)."""
        shapes = [(96, 64), (50, 75), (64, 64), (300, 200)]  # (w, h)

        def __getitem__(self, index):
            img, boxes, labels, voc = super().__getitem__(index)
            w, h = self.shapes[index]
            if index == 2:
                boxes, labels = boxes[:0], labels[:0]
            return (np.ascontiguousarray(img[:h, :w]), boxes, labels, voc)

    ds = Mixed(transform=TrainAugmentor(multiscale=(32, 64, 32), seed=4),
               size=4, imsize=300, seed=5)
    items = [ds[i] for i in range(4)]
    img_u8, sizes, coef, T, boxes, labels, dicts = \
        ds.collate_device_aug(items)
    # 300 x 200 exceeds 128 on its longer side: reduced by 3 to 100 x 67
    assert sizes.tolist() == [[64, 96], [75, 50], [64, 64], [67, 100]]
    assert img_u8.shape == (4, 75, 100, 3) and img_u8.dtype == torch.uint8
    assert not img_u8[0, 64:].any() and not img_u8[1, :, 50:].any()
    assert sizes.dtype == torch.int32
    assert coef.shape == (4, 5) and coef.dtype == torch.float32
    assert torch.isfinite(coef).all()
    assert T == 64 and isinstance(T, int)
    assert boxes.dtype == torch.float32 and labels.dtype == torch.int32
    assert boxes.shape[0] == 4 and boxes.shape[1] % 8 == 0
    assert (labels[2] < 0).all()
    assert boxes.min() >= 0 and boxes.max() <= T
    assert [d['annotation']['filename'] for d in dicts] == \
        [it[3]['annotation']['filename'] for it in items]

    args = build_parser(['--train-flag', '--device-augment'])
    cpu = torch.device('cpu')
    out = prepare_batch((img_u8, sizes, coef, T, boxes, labels), cpu, args,
                        False, False)
    want_shapes = [(4, 3, 64, 64), (4, 2, 16, 16), (4, 2, 16, 16),
                   (4, 2, 16, 16), (4, 1, 16, 16)]
    assert [tuple(t.shape) for t in out] == want_shapes
    assert all(t.dtype == torch.float32 and torch.isfinite(t).all()
               for t in out)
    assert not out[4][2].any() and out[4].sum() > 0
    # the seam on CPU is the oracle, and the image is its normalised form
    q = opsF.augment_images(img_u8, sizes, coef, T)
    assert q.dtype == torch.uint8 and q.shape == (4, 64, 64, 3)
    assert torch.equal(out[0], eager.normalize_images(q, args.pretrained))


def test_main_trains_with_device_augment(tmp_path):
    save = str(tmp_path / 'run')
    env = dict(os.environ)
    env['PYTHONPATH'] = REPO
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, 'main.py'), '--train-flag',
         '--synthetic', '--synthetic-size', '4', '--gpu-no', '-1',
         '--batch-size', '2', '--end-epoch', '1', '--num-workers', '0',
         '--imsize', '64', '--multiscale', '64', '64', '64', '--num-stack',
         '1', '--hourglass-inch', '16', '--print-interval', '1',
         '--random-seed', '7', '--device-augment', '--save-path', save],
        cwd=str(tmp_path), env=env, capture_output=True, text=True,
        timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert 'Iteration [   2/   2]' in r.stdout, r.stdout[-2000:]
    assert 'nan' not in r.stdout.lower()
    assert os.path.isfile(os.path.join(save, 'check_point_1.pth'))
    with open(os.path.join(save, 'argument.txt')) as f:
        text = f.read()
    assert 'device_augment: True' in text and 'device_encode: True' in text
