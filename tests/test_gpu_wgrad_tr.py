"""Transposed-read bf16 wgrad (ops/csrc/wgrad_tr.hip) against the
register-transpose kernel it replaces and against F.conv2d.

Both kernels take their chunk length from the same rule of the host
function (a function of the shape and RTHD_WGRAD_CHUNK only), so a pair of
calls on one shape always runs with equal chunk length; with that the new
kernel feeds every accumulator the same MFMA sequence and must be BITWISE
equal to the old one.

At these sizes the default rule gives 128-px chunks, i.e. at most two 64-px
K-steps, both issued by the kernel's prologue. MANY_STEPS therefore forces
longer chunks (or uses shapes whose rule gives them): 8 to 32 K-steps, so
the 3-deep ring wraps several times, loads issued inside the loop overwrite
buffers other waves have just read, and the incremental pixel walk advances
many times, over images whose pixel count (144, 400) is no divisor or
multiple of the K-step.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last

# (Cin, Cout, k, stride, pad, H, B)
SHAPES = [
    (64, 32, 3, 1, 1, 12, 2),    # M=288: no multiple of 128; Cout below tile
    (128, 128, 3, 1, 1, 16, 2),  # full tile
    (128, 128, 1, 1, 0, 16, 2),  # 1x1
    (64, 128, 3, 1, 1, 16, 2),   # Cin below Cout
    (152, 64, 1, 1, 0, 32, 2),   # stem column case, channel tail of 24
    (128, 8, 1, 1, 0, 16, 2),    # padded head
    (128, 128, 3, 1, 1, 8, 1),   # M=64: below one K block, mostly halo
    (128, 128, 2, 2, 0, 16, 2),  # the non-SAME address path
]

# ((Cin, Cout, k, stride, pad, H, B), RTHD_WGRAD_CHUNK or None, K-steps)
MANY_STEPS = [
    ((128, 128, 3, 1, 1, 16, 2), 512, 8),     # the full tile, ring wraps twice
    ((64, 32, 3, 1, 1, 12, 4), 512, 8),       # 144 px/image; chunks 512 + 64
    ((72, 136, 3, 1, 1, 20, 3), 1024, 16),    # 400 px/image; 8-channel tails
    ((64, 64, 3, 2, 1, 40, 3), 640, 10),      # strided map with a halo
    ((152, 64, 1, 1, 0, 64, 2), None, 32),    # 8192 px: the 1x1 2048-px rule
    # 65536 px: the XCD cell remap is on, 927 blocks (927 % 8 = 7)
    ((8, 8, 3, 1, 1, 64, 16), None, 10),
]


def _C():
    from real_time_helmet_detection_amd.ops import _backend
    return _backend.require_ext()


def rel_err(got, want):
    got = got.detach().float().cpu()
    want = want.detach().float().cpu()
    denom = want.abs().max().clamp(min=1e-6)
    return ((got - want).abs().max() / denom).item()


def _chunk_steps(cfg):
    """64-px K-steps of a full chunk under the host's chunk rule and the
    current RTHD_WGRAD_CHUNK."""
    cin, cout, k, stride, pad, h, b = cfg
    ho = (h + 2 * pad - k) // stride + 1
    m = b * ho * ho
    length = _C().wgrad_bf16_chunk_len(cin, cout, k * k, m)
    return -(-min(length, m) // 64)


@functools.lru_cache(maxsize=None)
def _case(cfg):
    """Inputs on the GPU, the F.conv2d weight gradient, and the old
    kernel's result at the default chunk length — computed once."""
    cin, cout, k, stride, pad, h, b = cfg
    torch.manual_seed(31)
    x = torch.randn(b, cin, h, h).to(torch.bfloat16).float()
    w = torch.randn(cout, cin, k, k, requires_grad=True)
    y = F.conv2d(x, w, None, stride=stride, padding=pad)
    dy = torch.randn_like(y).to(torch.bfloat16).float()
    y.backward(dy)
    xg = x.to('cuda', torch.bfloat16).contiguous(memory_format=CL)
    dyg = dy.to('cuda', torch.bfloat16).contiguous(memory_format=CL)
    old = _C().wgrad_bf16_fast(xg, dyg, k, k, stride, pad, variant='regt')
    return xg, dyg, w.grad.detach(), old


def test_lds_tr16_lane_map():
    """ds_read_b64_tr_b16 delivers the 16x16x32 operand layout: lane l,
    element j = image[k = 8*(l>>4) + j][m = 16*cb + (l&15)]."""
    got = _C().lds_tr16_selftest().cpu().to(torch.int64)
    lane = torch.arange(64).view(1, 64, 1)
    j = torch.arange(8).view(1, 1, 8)
    cb = torch.arange(4).view(4, 1, 1)
    want = (8 * (lane >> 4) + j) * 64 + 16 * cb + (lane & 15)
    assert got.shape == (4, 64, 8)
    assert torch.equal(got, want), got[0, :, :].tolist()


@pytest.mark.parametrize('cfg', SHAPES)
def test_bitwise_equal_to_register_transpose(cfg):
    cin, cout, k, stride, pad, h, b = cfg
    xg, dyg, _, old = _case(cfg)
    new = _C().wgrad_bf16_fast(xg, dyg, k, k, stride, pad, variant='tr')
    assert new.shape == old.shape and new.stride() == old.stride()
    assert torch.equal(new, old)


def test_bitwise_equal_many_chunks(monkeypatch):
    """RTHD_WGRAD_CHUNK=128: many chunks, a chunk boundary inside an image
    row (16-px rows, 128-px chunks start mid-image)."""
    cfg = (128, 128, 3, 1, 1, 16, 2)
    xg, dyg, want, _ = _case(cfg)
    monkeypatch.setenv('RTHD_WGRAD_CHUNK', '128')
    old = _C().wgrad_bf16_fast(xg, dyg, 3, 3, 1, 1, variant='regt')
    new = _C().wgrad_bf16_fast(xg, dyg, 3, 3, 1, 1, variant='tr')
    assert torch.equal(new, old)
    assert rel_err(old, want) < 0.03


@pytest.mark.parametrize('cfg,chunk,steps', MANY_STEPS)
def test_many_k_steps(cfg, chunk, steps, monkeypatch):
    """Steady state of the ring: bitwise against the old kernel at the same
    chunk length, parity against F.conv2d, and two calls bitwise equal."""
    cin, cout, k, stride, pad, h, b = cfg
    xg, dyg, want, _ = _case(cfg)
    if chunk:
        monkeypatch.setenv('RTHD_WGRAD_CHUNK', str(chunk))
    assert _chunk_steps(cfg) == steps >= 8
    old = _C().wgrad_bf16_fast(xg, dyg, k, k, stride, pad, variant='regt')
    new = _C().wgrad_bf16_fast(xg, dyg, k, k, stride, pad, variant='tr')
    again = _C().wgrad_bf16_fast(xg, dyg, k, k, stride, pad, variant='tr')
    assert torch.equal(new, old)
    assert torch.equal(again, new)
    assert rel_err(new, want) < 0.03


@pytest.mark.parametrize('cfg', SHAPES)
def test_parity_and_determinism(cfg):
    cin, cout, k, stride, pad, h, b = cfg
    xg, dyg, want, _ = _case(cfg)
    a = _C().wgrad_bf16_fast(xg, dyg, k, k, stride, pad, variant='tr')
    b2 = _C().wgrad_bf16_fast(xg, dyg, k, k, stride, pad, variant='tr')
    assert torch.equal(a, b2)
    assert rel_err(a, want) < 0.03


def test_default_dispatch_and_env(monkeypatch):
    """Default dispatch: the new kernel for aligned channels above 4096 px,
    the old one otherwise and wherever RTHD_WGRAD_REGT=1 (read per call).
    The default call on a shape the new kernel takes is bitwise the old
    kernel's result; a misuse of `variant` is an error."""
    C = _C()
    monkeypatch.delenv('RTHD_WGRAD_REGT', raising=False)
    assert C.wgrad_bf16_choice(152, 64, 8192) == 'tr'
    assert C.wgrad_bf16_choice(8, 8, 65536) == 'tr'
    assert C.wgrad_bf16_choice(128, 128, 4096) == 'regt'
    assert C.wgrad_bf16_choice(3, 64, 8192) == 'regt'
    assert C.wgrad_bf16_choice(128, 6, 8192) == 'regt'

    for cfg in [(152, 64, 1, 1, 0, 64, 2), (8, 8, 3, 1, 1, 64, 16)]:
        cin, cout, k, stride, pad, h, b = cfg
        xg, dyg, want, old = _case(cfg)
        got = C.wgrad_bf16_fast(xg, dyg, k, k, stride, pad)
        assert torch.equal(got, old)
        assert rel_err(got, want) < 0.03

    monkeypatch.setenv('RTHD_WGRAD_REGT', '1')
    assert C.wgrad_bf16_choice(152, 64, 8192) == 'regt'
    cfg = (152, 64, 1, 1, 0, 64, 2)
    xg, dyg, _, old = _case(cfg)
    assert torch.equal(C.wgrad_bf16_fast(xg, dyg, 1, 1, 1, 0), old)
    monkeypatch.setenv('RTHD_WGRAD_REGT', '0')
    assert C.wgrad_bf16_choice(152, 64, 8192) == 'tr'

    x3 = torch.randn(2, 3, 8, 8, device='cuda', dtype=torch.bfloat16) \
        .contiguous(memory_format=CL)
    d3 = torch.randn(2, 8, 8, 8, device='cuda', dtype=torch.bfloat16) \
        .contiguous(memory_format=CL)
    with pytest.raises(RuntimeError):
        C.wgrad_bf16_fast(x3, d3, 1, 1, 1, 0, variant='tr')
    with pytest.raises(RuntimeError):
        C.wgrad_bf16_fast(xg, dyg, 1, 1, 1, 0, variant='nope')
