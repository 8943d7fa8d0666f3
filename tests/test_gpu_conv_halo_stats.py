"""BN statistics from the halo conv's output tile (conv_fwd_halo_stats +
bn_stats_from_parts) against the halo conv followed by bn_stats.

Error bounds are derived, not tuned. A channel's device sum adds n bf16
values (n = pixels per channel) in fp32 in some fixed grouping; whatever
the grouping, first-order fp32 summation error is at most
n * 2^-24 * sum|v| (every one of the < n additions rounds a partial sum
that is at most sum|v| in magnitude). The squares of bf16 values are exact
in fp32 (8 x 8 significand bits), so the same bound holds for the sum of
squares with v^2 in place of v. Everything behind the sums (mean, rstd,
running statistics) is a handful of fp32 scalar operations whose
first-order sensitivities are written out in `_finish_bounds`.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

CL = torch.channels_last
U = 2.0 ** -24          # fp32 unit roundoff
EPS = 1e-5
MOM = 0.1
TH, TW = 8, 16          # the halo kernel's tile
SENTINEL = -12345.0

SHAPES = [(8, 16), (16, 32), (24, 48)]   # 1, 4 and 9 tiles per image
CINS = [64, 128]
COUTS = [128, 64, 136]  # full N tile, padded N tile, two N blocks
B = 2


def _C():
    from real_time_helmet_detection_amd.ops import _backend
    return _backend.require_ext()


_cases = {}


def _case(hw, cin, cout):
    """Inputs and the forced-halo reference of one configuration, built once
    and shared (never modified) by every test that needs them."""
    key = (hw, cin, cout)
    if key not in _cases:
        h, w = hw
        g = torch.Generator().manual_seed(1000 * h + 10 * cin + cout)
        x = torch.randn(B, cin, h, w, generator=g).to('cuda', torch.bfloat16)
        x = x.contiguous(memory_format=CL)
        wt = (torch.randn(cout, cin, 3, 3, generator=g) * 0.05).cuda()
        ones = torch.ones(cout, device='cuda')
        bias = (torch.randn(cout, generator=g) * 0.5).cuda()
        wpk = _C().pack_weights(wt, False, True)
        y = _C().conv_fwd_halo(x, wpk, ones, bias, None, 3, 3, 1, 1, cout, 0)
        _cases[key] = dict(x=x, wpk=wpk, ones=ones, bias=bias, y=y,
                           tiles=B * (h // TH) * (w // TW), n=B * h * w,
                           cout=cout)
    return _cases[key]


def _run(c, p1=None, p2=None):
    return _C().conv_fwd_halo_stats(c['x'], c['wpk'], c['ones'], c['bias'],
                                    3, 3, 1, 1, c['cout'], 0, p1, p2)


def _finish(c, p1, p2):
    rm = torch.full((c['cout'],), 0.25, device='cuda')
    rv = torch.full((c['cout'],), 1.5, device='cuda')
    mean, rstd = _C().bn_stats_from_parts(p1, p2, rm, rv, MOM, EPS, c['n'])
    return mean, rstd, rm, rv


def _exact_sums(y):
    """fp64 sum|v|, sum v, sum v^2 per channel of y's bf16 values."""
    v = y.permute(0, 2, 3, 1).reshape(-1, y.shape[1]).double()
    return v.abs().sum(0), v.sum(0), (v * v).sum(0)


def _finish_bounds(c):
    """Per-channel bounds on |a - b| for two fp32 evaluations of mean, rstd,
    running mean and running var whose sums each carry the summation bound.
    ULPS fp32 roundings are allowed for the scalar operations behind the
    sums (a division, a multiply-subtract, rsqrt, the momentum blend)."""
    ULPS = 4
    n = c['n']
    sabs, s1, s2 = _exact_sums(c['y'])
    mean = s1 / n
    ex2 = s2 / n
    var = (ex2 - mean * mean).clamp(min=0)
    rstd = (var + EPS).rsqrt()
    # two sums, each within n*U*sum|v| of the exact one
    d_mean = 2 * n * U * sabs / n + ULPS * U * mean.abs()
    d_var = (2 * n * U * s2 / n + 2 * mean.abs() * d_mean +
             ULPS * U * (ex2 + mean * mean))
    d_rstd = 0.5 * rstd ** 3 * d_var + ULPS * U * rstd
    unbias = n / (n - 1.0)
    d_rm = MOM * d_mean + ULPS * U * (0.25 + mean.abs())
    d_rv = MOM * unbias * d_var + ULPS * U * (1.5 + var * unbias)
    return d_mean, d_rstd, d_rm, d_rv


CONFIGS = [(hw, cin, cout) for hw in SHAPES for cin in CINS
           for cout in COUTS]


@pytest.mark.parametrize('hw,cin,cout', CONFIGS)
def test_output_and_partials(hw, cin, cout):
    c = _case(hw, cin, cout)
    tiles = c['tiles']
    # over-allocated, sentinel-filled: 3 spare rows, 8 spare columns
    p1 = torch.full((tiles + 3, cout + 8), SENTINEL, device='cuda')
    p2 = torch.full((tiles + 3, cout + 8), SENTINEL, device='cuda')
    y, q1, q2 = _run(c, p1, p2)
    torch.cuda.synchronize()

    # the conv output is the halo kernel's, bit for bit
    assert torch.equal(y, c['y'])

    # nothing outside [tiles][Cout] is touched, everything inside is written
    for p in (p1, p2):
        assert (p[tiles:] == SENTINEL).all()
        assert (p[:, cout:] == SENTINEL).all()
        assert not (p[:tiles, :cout] == SENTINEL).any()
    assert q1.data_ptr() == p1.data_ptr() and q2.data_ptr() == p2.data_ptr()

    # partial rows, summed in fp64 on the host, against fp64 sums of y
    sabs, s1, s2 = _exact_sums(c['y'])
    n = c['n']
    got1 = p1[:tiles, :cout].double().sum(0)
    got2 = p2[:tiles, :cout].double().sum(0)
    err1 = (got1 - s1).abs()
    err2 = (got2 - s2).abs()
    print('max err/bound sum %.3g sumsq %.3g' % (
        (err1 / (n * U * sabs)).max().item(),
        (err2 / (n * U * s2)).max().item()))
    assert (err1 <= n * U * sabs).all()
    assert (err2 <= n * U * s2).all()


@pytest.mark.parametrize('hw,cin,cout', CONFIGS)
def test_deterministic(hw, cin, cout):
    c = _case(hw, cin, cout)
    _, a1, a2 = _run(c)
    fa = _finish(c, a1, a2)
    _, b1, b2 = _run(c)
    fb = _finish(c, b1, b2)
    assert torch.equal(a1, b1) and torch.equal(a2, b2)
    for u, v in zip(fa, fb):
        assert torch.equal(u, v)


@pytest.mark.parametrize('hw,cin,cout', CONFIGS)
def test_finish_matches_bn_stats(hw, cin, cout):
    c = _case(hw, cin, cout)
    _, p1, p2 = _run(c)
    mean, rstd, rm, rv = _finish(c, p1, p2)
    wrm = torch.full((cout,), 0.25, device='cuda')
    wrv = torch.full((cout,), 1.5, device='cuda')
    wmean, wrstd = _C().bn_stats(c['y'], wrm, wrv, MOM, EPS)
    bounds = _finish_bounds(c)
    pairs = ((mean, wmean), (rstd, wrstd), (rm, wrm), (rv, wrv))
    for name, (got, want), bound in zip(('mean', 'rstd', 'run_mean',
                                         'run_var'), pairs, bounds):
        err = (got.double() - want.double()).abs()
        print('%s max err/bound %.3g' % (name, (err / bound).max().item()))
        assert (err <= bound).all(), name


@pytest.mark.parametrize('hw,cin,cout', CONFIGS)
def test_capture_replay_equals_eager(hw, cin, cout):
    c = _case(hw, cin, cout)
    rm = torch.empty(cout, device='cuda')
    rv = torch.empty(cout, device='cuda')

    def body():
        y, p1, p2 = _run(c)
        mean, rstd = _C().bn_stats_from_parts(p1, p2, rm, rv, MOM, EPS,
                                              c['n'])
        return [y, p1, p2, mean, rstd]

    rm.fill_(0.25)
    rv.fill_(1.5)
    want = [t.clone() for t in body()]
    want_rm, want_rv = rm.clone(), rv.clone()
    torch.cuda.synchronize()

    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = body()
    for _ in range(2):
        rm.fill_(0.25)
        rv.fill_(1.5)
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, want):
            assert torch.equal(a, b)
        assert torch.equal(rm, want_rm) and torch.equal(rv, want_rv)


def test_conv_fwd_stats_rule_on_tile_count():
    """conv_fwd_stats with a tile threshold: a halo shape at the threshold
    returns one partial row per tile, one tile short of it returns the plain
    conv; y is the same either way. (Which variant a shape runs is the
    autotuner's choice; the row count says which one ran.)"""
    C = _C()
    cout = 128
    g = torch.Generator().manual_seed(5)
    x = torch.randn(16, 128, 64, 64, generator=g).to('cuda', torch.bfloat16)
    x = x.contiguous(memory_format=CL)
    wt = (torch.randn(cout, 128, 3, 3, generator=g) * 0.05).cuda()
    wpk = C.pack_weights(wt, False, True)
    ones = torch.ones(cout, device='cuda')
    zeros = torch.zeros(cout, device='cuda')
    tiles = 16 * (64 // TH) * (64 // TW)
    want = C.conv_fwd(x, wpk, ones, zeros, None, 3, 3, 1, 1, cout, 0)
    on = C.conv_fwd_stats(x, wpk, ones, zeros, 3, 3, 1, 1, cout, 0, tiles)
    off = C.conv_fwd_stats(x, wpk, ones, zeros, 3, 3, 1, 1, cout, 0,
                           tiles + 1)
    assert len(off) == 1
    assert torch.equal(off[0], want)
    assert torch.equal(on[0], want)
    if len(on) == 3:
        assert tuple(on[1].shape) == (tiles, cout)
        mean, rstd = C.bn_stats_from_parts(on[1], on[2], None, None, MOM,
                                           EPS, x.numel() // 128)
        wmean, wrstd = C.bn_stats(want, None, None, MOM, EPS)
        d_mean, d_rstd, _, _ = _finish_bounds(
            dict(y=want, n=x.numel() // 128))
        assert ((mean.double() - wmean.double()).abs() <= d_mean).all()
        assert ((rstd.double() - wrstd.double()).abs() <= d_rstd).all()
