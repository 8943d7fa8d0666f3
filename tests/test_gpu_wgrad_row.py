"""Tap-row bf16 wgrad (ops/csrc/wgrad_row.hip) against the transposed-read
kernel it is built on and against F.conv2d.

The row kernel keeps the chunk boundaries, the k-slot of every pixel and the
MFMA of variant 'tr', and the element it masks in a register is the zero the
zero page delivers there, so under one forced RTHD_WGRAD_CHUNK both kernels
feed every accumulator the same MFMA sequence: the results must be BITWISE
equal. The shapes are the smallest at which each mechanism can go wrong
(apron across a chunk boundary, both edges in every k-block, ring wrap,
channel tails); the exact edge test makes a wrapped product or a mask on the
wrong k-slot a wrong integer.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last

# ((Cin, Cout, H, W, B), RTHD_WGRAD_CHUNK); 3x3 stride 1 pad 1
CASES = [
    ((64, 64, 8, 32, 2), 128),      # narrowest row: both edges per k-block
    ((128, 128, 32, 32, 2), 512),   # full tiles, 8 K-steps
    ((64, 128, 24, 64, 3), 1024),   # 16 K-steps, chunks end inside an image
    ((72, 136, 8, 64, 2), 128),     # 8-channel tails in both operands
    ((128, 128, 2, 256, 2), 128),   # chunk boundaries inside an image row
]

EDGE_CASES = [(64, 64, 8, 32, 2), (64, 64, 4, 64, 2)]


def _C():
    from real_time_helmet_detection_amd.ops import _backend
    return _backend.require_ext()


def rel_err(got, want):
    got = got.detach().float().cpu()
    want = want.detach().float().cpu()
    denom = want.abs().max().clamp(min=1e-6)
    return ((got - want).abs().max() / denom).item()


def _conv_grad(x, dy, cout, dtype):
    """F.conv2d weight gradient on the CPU in `dtype`."""
    x = x.to(dtype)
    w = torch.zeros(cout, x.shape[1], 3, 3, dtype=dtype, requires_grad=True)
    y = F.conv2d(x, w, None, stride=1, padding=1)
    y.backward(dy.to(dtype))
    return w.grad.detach()


@functools.lru_cache(maxsize=None)
def _case(cfg):
    """Inputs on the GPU and the F.conv2d weight gradient — computed once."""
    cin, cout, h, w, b = cfg
    torch.manual_seed(37)
    x = torch.randn(b, cin, h, w).to(torch.bfloat16).float()
    dy = torch.randn(b, cout, h, w).to(torch.bfloat16).float()
    want = _conv_grad(x, dy, cout, torch.float32)
    xg = x.to('cuda', torch.bfloat16).contiguous(memory_format=CL)
    dyg = dy.to('cuda', torch.bfloat16).contiguous(memory_format=CL)
    return xg, dyg, want


@pytest.mark.parametrize('cfg,chunk', CASES)
def test_bitwise_equal_to_tr(cfg, chunk, monkeypatch):
    """Same forced chunk length: bitwise equal to variant 'tr', parity with
    F.conv2d, two calls bitwise equal."""
    cin, cout, h, w, b = cfg
    xg, dyg, want = _case(cfg)
    monkeypatch.setenv('RTHD_WGRAD_CHUNK', str(chunk))
    C = _C()
    assert C.wgrad_row_chunk_len(cin, cout, b * h * w) == chunk
    assert C.wgrad_bf16_chunk_len(cin, cout, 9, b * h * w) == chunk
    tr = C.wgrad_bf16_fast(xg, dyg, 3, 3, 1, 1, variant='tr')
    row = C.wgrad_bf16_fast(xg, dyg, 3, 3, 1, 1, variant='row')
    again = C.wgrad_bf16_fast(xg, dyg, 3, 3, 1, 1, variant='row')
    assert row.shape == tr.shape and row.stride() == tr.stride()
    assert torch.equal(row, tr)
    assert torch.equal(again, row)
    assert rel_err(row, want) < 0.03


@pytest.mark.parametrize('cfg', EDGE_CASES)
def test_edges_exact(cfg):
    """Integer inputs in [-3, 3], nonzero only in columns 0 and W-1 of both
    X and dY: every sum is a small integer, exact in fp32 in any order, so
    the result must equal the float64 gradient. The product a wrapped read
    would add (column W-1 of the row above times column 0) is nonzero."""
    cin, cout, h, w, b = cfg
    torch.manual_seed(41)
    x = torch.zeros(b, cin, h, w)
    dy = torch.zeros(b, cout, h, w)
    for t, c in ((x, cin), (dy, cout)):
        for col in (0, w - 1):
            t[:, :, :, col] = torch.randint(-3, 4, (b, c, h)).float()
    want = _conv_grad(x, dy, cout, torch.float64)
    assert want.abs().max().item() < 2 ** 24
    xg = x.to('cuda', torch.bfloat16).contiguous(memory_format=CL)
    dyg = dy.to('cuda', torch.bfloat16).contiguous(memory_format=CL)
    got = _C().wgrad_bf16_fast(xg, dyg, 3, 3, 1, 1, variant='row')
    assert torch.equal(got.cpu().double(), want)


def test_dispatch(monkeypatch):
    C = _C()
    monkeypatch.delenv('RTHD_WGRAD_ROW', raising=False)
    monkeypatch.delenv('RTHD_WGRAD_REGT', raising=False)

    def choice(cin, cout, k, stride, pad, h, w, b):
        return C.wgrad_bf16_choice_geo(cin, cout, k, k, stride, pad, h, w, b)

    assert choice(128, 128, 3, 1, 1, 128, 128, 16) == 'row'
    assert choice(64, 128, 3, 1, 1, 256, 256, 16) == 'row'
    assert choice(128, 128, 1, 1, 0, 128, 128, 16) == 'tr'
    assert choice(128, 128, 3, 2, 1, 128, 128, 16) == 'tr'
    assert choice(128, 128, 3, 1, 1, 48, 48, 16) == 'tr'
    assert choice(8, 128, 3, 1, 1, 128, 128, 16) == 'tr'
    monkeypatch.setenv('RTHD_WGRAD_ROW', '0')
    assert choice(128, 128, 3, 1, 1, 128, 128, 16) == 'tr'
    assert choice(64, 128, 3, 1, 1, 256, 256, 16) == 'tr'
    monkeypatch.delenv('RTHD_WGRAD_ROW')

    # ineligible shapes under variant='row': 1x1, stride 2, Wo = 48
    for cin, cout, k, stride, pad, h in [(64, 64, 1, 1, 0, 32),
                                         (64, 64, 3, 2, 1, 64),
                                         (64, 64, 3, 1, 1, 48)]:
        ho = (h + 2 * pad - k) // stride + 1
        x = torch.randn(2, cin, h, h, device='cuda', dtype=torch.bfloat16) \
            .contiguous(memory_format=CL)
        d = torch.randn(2, cout, ho, ho, device='cuda',
                        dtype=torch.bfloat16).contiguous(memory_format=CL)
        with pytest.raises(RuntimeError):
            C.wgrad_bf16_fast(x, d, k, k, stride, pad, variant='row')
