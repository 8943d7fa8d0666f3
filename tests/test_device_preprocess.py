"""--device-preprocess on the CPU: the eager oracle ops.eager.resize_images
against Pillow and against the evaluation collate bit for bit, the
collate_frames batch form, evaluate_step with the flag off and on, and the
flag / argument checks. The gfx950 kernel is compared with this oracle in
tests/test_gpu_preprocess.py."""

import functools

import numpy as np
import pytest
import torch
from PIL import Image

from real_time_helmet_detection_amd import ops
from real_time_helmet_detection_amd.config import (ARCH_FLAGS, build_parser,
                                                   update_arguments_for_eval)
from real_time_helmet_detection_amd.data import VOC, TestAugmentor
from real_time_helmet_detection_amd.data import voc as voc_mod
from real_time_helmet_detection_amd.ops import eager
from real_time_helmet_detection_amd.ops import functional as opsF
from real_time_helmet_detection_amd.utils import get_normalizer

# (H, W, T): down- and upscales, identity, one-axis-only, 1x1, ratio ~14
CASES = [(37, 53, 16), (16, 16, 16), (9, 70, 32), (100, 7, 32),
         (270, 480, 64), (5, 5, 32), (33, 32, 32), (1, 1, 8), (129, 64, 64),
         (200, 260, 24)]

XML = """<annotation>
  <filename>%s.jpg</filename>
  <size><width>%d</width><height>%d</height><depth>3</depth></size>
  <object><name>hat</name>
    <bndbox><xmin>10</xmin><ymin>20</ymin><xmax>50</xmax><ymax>60</ymax></bndbox>
  </object>
  <object><name>person</name>
    <bndbox><xmin>60</xmin><ymin>5</ymin><xmax>90</xmax><ymax>70</ymax></bndbox>
  </object>
</annotation>"""

TREE_SIZES_WH = [(200, 100), (96, 150), (64, 64)]
T_TREE = 64


def _make_voc_root(tmp_path):
    """tests/test_data.py's helper, with three noise images of different
    sizes."""
    root = tmp_path / 'VOC2028'
    (root / 'JPEGImages').mkdir(parents=True)
    (root / 'Annotations').mkdir()
    (root / 'ImageSets/Main').mkdir(parents=True)
    rng = np.random.RandomState(11)
    names = []
    for i, (w, h) in enumerate(TREE_SIZES_WH):
        name = '%06d' % i
        names.append(name)
        Image.fromarray(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)).save(
            root / 'JPEGImages' / (name + '.jpg'))
        (root / 'Annotations' / (name + '.xml')).write_text(
            XML % (name, w, h))
    (root / 'ImageSets/Main/trainval.txt').write_text('\n'.join(names))
    (root / 'ImageSets/Main/test.txt').write_text('\n'.join(names))
    return str(root)


@pytest.fixture(scope='module')
def voc_root(tmp_path_factory):
    return _make_voc_root(tmp_path_factory.mktemp('voc'))


def _dataset(root, pretrained='imagenet'):
    return VOC(root=root, transform=TestAugmentor(T_TREE), image_set='test',
               pretrained=pretrained, normalized_coord=False, num_cls=2)


@functools.lru_cache(maxsize=None)
def _group(T):
    """All CASES of one T as one batch: (canvas, sizes, [image arrays]).
    The canvas outside each image is 255s and random bytes, not zeros."""
    rng = np.random.RandomState(100 + T)
    hw = [(h, w) for h, w, t in CASES if t == T]
    hmax = max(h for h, _ in hw) + 1
    wmax = max(w for _, w in hw) + 2
    canvas = rng.randint(0, 256, (len(hw), hmax, wmax, 3), dtype=np.uint8)
    canvas[:, ::2] = 255
    imgs = []
    for i, (h, w) in enumerate(hw):
        im = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
        canvas[i, :h, :w] = im
        imgs.append(im)
    return (torch.from_numpy(canvas),
            torch.tensor(hw, dtype=torch.int32), imgs)


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16,
                                4: torch.int32}[t.element_size()])


@pytest.mark.parametrize('T', sorted({t for _, _, t in CASES}))
def test_oracle_equals_pillow_bitwise(T):
    canvas, sizes, imgs = _group(T)
    got = opsF.resize_images(canvas, sizes, T)
    assert got.dtype == torch.uint8 and got.shape == (len(imgs), T, T, 3)
    for i, im in enumerate(imgs):
        want = np.asarray(Image.fromarray(im).resize((T, T), Image.BILINEAR))
        assert np.array_equal(got[i].numpy(), want), im.shape


@pytest.mark.parametrize('pretrained', ['imagenet', 'scratch'])
def test_normalised_equals_evaluation_collate_bitwise(pretrained):
    T = 32
    canvas, sizes, imgs = _group(T)
    # the collate arithmetic: TestAugmentor, /255, Normalizer
    resized, _, _ = TestAugmentor(T)(imgs, [np.zeros((0, 4))] * len(imgs),
                                     [np.zeros(0)] * len(imgs))
    norm = get_normalizer(pretrained=pretrained)
    want = torch.stack([
        norm(torch.from_numpy(
            np.ascontiguousarray(im.transpose(2, 0, 1))).float() / 255.0)
        for im in resized])
    got = opsF.resize_images(canvas, sizes, T, pretrained)
    assert got.dtype == torch.float32 and got.shape == (len(imgs), 3, T, T)
    assert got.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(_bits(got), _bits(want))
    bf = opsF.resize_images(canvas, sizes, T, pretrained, torch.bfloat16)
    assert bf.dtype == torch.bfloat16
    assert torch.equal(_bits(bf), _bits(got.to(torch.bfloat16)))
    # and ops.resize_images is the same dispatch
    assert torch.equal(ops.resize_images(canvas, sizes, T, pretrained), got)


def test_collate_frames_shapes_and_equality(voc_root):
    ds = _dataset(voc_root)
    batch = [ds[i] for i in range(3)]
    canvas, sizes, dicts = ds.collate_frames(batch)
    assert canvas.dtype == torch.uint8 and canvas.shape == (3, 150, 200, 3)
    assert sizes.dtype == torch.int32
    assert sizes.tolist() == [[h, w] for w, h in TREE_SIZES_WH]
    assert [d['annotation']['filename'] for d in dicts] == \
        ['%06d.jpg' % i for i in range(3)]
    for i, (w, h) in enumerate(TREE_SIZES_WH):
        assert np.array_equal(canvas[i, :h, :w].numpy(), batch[i][0])
    want = ds.collate_fn(batch)[0]
    got = opsF.resize_images(canvas, sizes, T_TREE, 'imagenet')
    assert torch.equal(_bits(got), _bits(want))


def test_collate_frames_worker_fallback(voc_root, monkeypatch):
    """Past the kernel's cap the worker resizes with Pillow and ships a
    T x T image; the device pass is the identity on it."""
    ds = _dataset(voc_root)
    batch = [ds[i] for i in range(3)]
    monkeypatch.setattr(voc_mod, 'DEVICE_RESIZE_MAX_RATIO', 1)
    canvas, sizes, _ = ds.collate_frames(batch)
    # every side above 64 is past the cap now: all three arrive 64 x 64
    assert canvas.shape == (3, T_TREE, T_TREE, 3)
    assert sizes.tolist() == [[T_TREE, T_TREE]] * 3
    got = opsF.resize_images(canvas, sizes, T_TREE, 'imagenet')
    assert torch.equal(_bits(got), _bits(ds.collate_fn(batch)[0]))
    monkeypatch.setattr(voc_mod, 'DEVICE_RESIZE_MAX_RATIO', 2)
    canvas, sizes, _ = ds.collate_frames(batch)
    # 200 and 150 are past 2 * 64; 96 x 150 falls back whole
    assert sizes.tolist() == [[T_TREE, T_TREE], [T_TREE, T_TREE],
                              [T_TREE, T_TREE]]
    monkeypatch.setattr(voc_mod, 'DEVICE_RESIZE_MAX_RATIO', 3)
    canvas, sizes, _ = ds.collate_frames(batch)
    assert sizes.tolist() == [[T_TREE, T_TREE], [150, 96], [64, 64]]
    got = opsF.resize_images(canvas, sizes, T_TREE, 'imagenet')
    assert torch.equal(_bits(got), _bits(ds.collate_fn(batch)[0]))


def run_evaluate_step(voc_root, device, flag, net):
    """evaluate_step over the tree -> (predictor inputs, predictions)."""
    from real_time_helmet_detection_amd.engine.evaluator import (
        Prediction, evaluate_step)
    argv = ['--imsize', str(T_TREE), '--conf-th', '0.01', '--batch-size', '2']
    args = build_parser(argv + (['--device-preprocess'] if flag else []))
    ds = _dataset(voc_root, args.pretrained)
    loader = torch.utils.data.DataLoader(
        ds, batch_size=args.batch_size, shuffle=False, num_workers=0,
        collate_fn=ds.collate_frames if flag else ds.collate_fn)
    predictor = Prediction(
        network=net, topk=20, scale_factor=4, conf_th=args.conf_th,
        nms='nms', nms_th=0.5).to(device)
    seen = []
    predictor.register_forward_pre_hook(
        lambda mod, inp: seen.append(inp[0].detach().clone()))
    return seen, evaluate_step(loader, predictor, device, args)


def test_evaluate_step_cpu_flag_off_equals_on(voc_root):
    from real_time_helmet_detection_amd.models import StackedHourglass
    torch.manual_seed(3)
    net = StackedHourglass(num_stack=1, in_ch=16, out_ch=6).eval()
    cpu = torch.device('cpu')
    in_off, pred_off = run_evaluate_step(voc_root, cpu, False, net)
    in_on, pred_on = run_evaluate_step(voc_root, cpu, True, net)
    assert len(in_off) == len(in_on) == 2
    for a, b in zip(in_off, in_on):
        assert a.shape == b.shape and torch.equal(_bits(a), _bits(b))
    assert list(pred_off) == list(pred_on) == \
        ['%06d.jpg' % i for i in range(3)]
    assert any(len(v) for v in pred_off.values())
    for key in pred_off:
        assert pred_off[key].dtype == pred_on[key].dtype
        assert np.array_equal(pred_off[key], pred_on[key])


def test_flags():
    assert build_parser([]).device_preprocess is False
    assert build_parser([]).raw_input is False
    assert build_parser(['--device-preprocess']).device_preprocess is True
    assert build_parser(['--raw-input']).raw_input is True
    assert 'device_preprocess' not in ARCH_FLAGS
    assert 'raw_input' not in ARCH_FLAGS
    args = update_arguments_for_eval(
        build_parser([]), {'device_preprocess': True, 'num_stack': 3})
    assert args.device_preprocess is False and args.num_stack == 3


def test_flag_is_ignored_in_training(capsys):
    args = build_parser(['--train-flag', '--device-preprocess'])
    assert args.device_preprocess is False
    out = capsys.readouterr().out
    assert '--device-preprocess' in out and len(out.splitlines()) == 1


def test_host_size_checks():
    canvas = torch.zeros((2, 10, 12, 3), dtype=torch.uint8)
    ok = torch.tensor([[10, 12], [1, 1]], dtype=torch.int32)
    assert opsF.resize_images(canvas, ok, 4).shape == (2, 4, 4, 3)
    for bad in ([[11, 12], [1, 1]], [[10, 13], [1, 1]], [[10, 12], [0, 1]],
                [[10, 12], [1, -1]]):
        with pytest.raises(ValueError):
            opsF.resize_images(canvas, torch.tensor(bad, dtype=torch.int32),
                               4)
    with pytest.raises(ValueError):
        opsF.resize_images(canvas, ok[:1], 4)
    with pytest.raises(ValueError):
        opsF.resize_images(canvas, ok, 0)
    assert eager.resize_images(canvas[:0], ok[:0], 4).shape == (0, 4, 4, 3)
