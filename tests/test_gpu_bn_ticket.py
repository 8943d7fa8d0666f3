"""Single-launch BN reductions and the paired weight pack (run on MI355X).

The reduce kernels of ``bn.hip`` finish their own reduction with arrival
tickets; ``RTHD_BN_STAGED=1`` selects the older three-launch path at call
time. Both sum the same partial rows in the same order, so everything here is
compared bitwise (``torch.equal``), never with a tolerance.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

CL = torch.channels_last


def _C():
    from real_time_helmet_detection_amd.ops import _backend
    return _backend.require_ext()


def _chunks(shape):
    """pick_chunks of bn.hip: ceil(M*C / 16384) clamped to [1, 1024]."""
    n = 1
    for d in shape:
        n *= d
    return max(1, min(1024, -(-n // 16384)))


# shape, dtype, intended chunk count (what each covers: see the ids)
CASES = [
    pytest.param((2, 64, 8, 8), torch.bfloat16, 1, id='1-single-block'),
    pytest.param((4, 128, 16, 16), torch.bfloat16, 8, id='8-one-level-max'),
    pytest.param((1, 128, 32, 33), torch.bfloat16, 9, id='9-two-level-min'),
    pytest.param((1, 64, 56, 57), torch.bfloat16, 13, id='13-uneven'),
    pytest.param((2, 8, 128, 130), torch.bfloat16, 17, id='17-one-octet'),
    pytest.param((2, 256, 24, 40), torch.bfloat16, 30, id='30-32-octets'),
    pytest.param((2, 24, 64, 120), torch.bfloat16, 23, id='23-scalar-bf16'),
    pytest.param((3, 33, 40, 50), torch.float32, 13, id='13-scalar-fp32'),
    pytest.param((4, 128, 192, 192), torch.bfloat16, 1024, id='1024-cap'),
]


def _inputs(shape, dtype, seed=0):
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)

    def rnd(*s):
        return torch.randn(*s, device='cuda', generator=g)

    c = shape[1]
    t = {
        'x': (rnd(*shape) * 1.5 + 0.3).to(dtype).contiguous(memory_format=CL),
        'dy': rnd(*shape).to(dtype).contiguous(memory_format=CL),
        'skip': rnd(*shape).to(dtype).contiguous(memory_format=CL),
        'gamma': rnd(c) * 0.5 + 1.0,
        'beta': rnd(c) * 0.1,
        'rm': rnd(c) * 0.1,
        'rv': rnd(c).abs() + 0.5,
    }
    return t


def _run_all(t):
    """Every reduction the ticket path touches, on fresh running stats."""
    C = _C()
    rm, rv = t['rm'].clone(), t['rv'].clone()
    mean, rstd = C.bn_stats(t['x'], rm, rv, 0.1, 1e-5)
    out = {'mean': mean, 'rstd': rstd, 'rm': rm, 'rv': rv}
    # backward on FIXED statistics so a broken bn_stats cannot hide here
    mu = t['rm']
    rs = torch.rsqrt(t['rv'] + 1e-5)
    for name, skip in (('bwd', None), ('bwd_skip', t['skip'])):
        res = C.bn_act_bwd(t['dy'], t['x'], mu, rs, t['gamma'], t['beta'], 1,
                           skip)
        for k, v in zip(('dx', 'dgamma', 'dbeta', 'dskip'), res):
            out[name + '.' + k] = v
    out['col_sum'] = C.col_sum(t['dy'])
    torch.cuda.synchronize()
    return out


def _assert_same(got, want, what=''):
    assert got.keys() == want.keys()
    for k in want:
        assert torch.equal(got[k], want[k]), '%s%s differs' % (what, k)


@pytest.mark.parametrize('shape,dtype,chunks', CASES)
def test_ticket_equals_staged(shape, dtype, chunks, monkeypatch):
    assert _chunks(shape) == chunks
    t = _inputs(shape, dtype)
    monkeypatch.setenv('RTHD_BN_STAGED', '1')
    want = _run_all(t)
    monkeypatch.delenv('RTHD_BN_STAGED')
    got = _run_all(t)
    assert set(want) >= {'mean', 'rstd', 'rm', 'rv', 'bwd.dx', 'bwd.dgamma',
                         'bwd.dbeta', 'bwd_skip.dskip', 'col_sum'}
    for v in want.values():
        assert torch.isfinite(v.float()).all()
    _assert_same(got, want)


def test_counter_reuse_back_to_back(monkeypatch):
    """20 calls alternating two shapes on one stream, no sync in between:
    the counters every launch leaves behind must be zero again."""
    monkeypatch.delenv('RTHD_BN_STAGED', raising=False)
    C = _C()
    shapes = [((1, 128, 32, 33), torch.bfloat16),
              ((2, 24, 64, 120), torch.bfloat16)]
    assert [_chunks(s) for s, _ in shapes] == [9, 23]
    ts = [_inputs(s, d, seed=i) for i, (s, d) in enumerate(shapes)]
    rs = [torch.rsqrt(t['rv'] + 1e-5) for t in ts]
    torch.cuda.synchronize()
    runs = [[], []]
    for i in range(20):
        t, r = ts[i % 2], rs[i % 2]
        mean, rstd = C.bn_stats(t['x'], None, None, 0.1, 1e-5)
        res = C.bn_act_bwd(t['dy'], t['x'], t['rm'], r, t['gamma'],
                           t['beta'], 1, t['skip'])
        runs[i % 2].append([mean, rstd] + list(res))
    torch.cuda.synchronize()
    for per_shape in runs:
        assert len(per_shape) == 10
        for later in per_shape[1:]:
            for a, b in zip(per_shape[0], later):
                assert torch.equal(a, b)


def test_graph_replay(monkeypatch):
    """Captured after one eager call (so the counter pool exists), the
    ticket path replays bitwise: counters are reset inside the graph."""
    monkeypatch.delenv('RTHD_BN_STAGED', raising=False)
    C = _C()
    shape = (1, 128, 32, 33)
    assert _chunks(shape) == 9
    t = _inputs(shape, torch.bfloat16)
    rm, rv = t['rm'].clone(), t['rv'].clone()

    def body():
        mean, rstd = C.bn_stats(t['x'], rm, rv, 0.1, 1e-5)
        y = C.bn_act_fwd(t['x'], mean, rstd, t['gamma'], t['beta'], 1,
                         t['skip'])
        dx, dgamma, dbeta, dskip = C.bn_act_bwd(
            t['dy'], t['x'], mean, rstd, t['gamma'], t['beta'], 1, t['skip'])
        return [mean, rstd, y, dx, dgamma, dbeta, dskip]

    want = [v.clone() for v in body()]
    want_rm, want_rv = rm.clone(), rv.clone()
    torch.cuda.synchronize()

    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = body()
    for _ in range(3):
        rm.copy_(t['rm'])
        rv.copy_(t['rv'])
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, want):
            assert torch.equal(a, b)
        assert torch.equal(rm, want_rm) and torch.equal(rv, want_rv)


def _strided_cl(w):
    return w.contiguous(memory_format=CL)


@pytest.mark.parametrize('fwd_bf16,dgrad_bf16', [
    (True, True), (False, False), (True, False), (False, True)])
@pytest.mark.parametrize('shape,layout', [
    ((128, 128, 3, 3), None),
    ((128, 64, 1, 1), None),
    ((6, 128, 1, 1), None),
    ((64, 128, 3, 3), _strided_cl),
])
def test_pack_weights_pair(shape, layout, fwd_bf16, dgrad_bf16):
    C = _C()
    torch.manual_seed(3)
    w = torch.randn(*shape, device='cuda')
    if layout is not None:
        w = layout(w)
        assert not w.is_contiguous()
    pk, pk_t = C.pack_weights_pair(w, fwd_bf16, dgrad_bf16)
    want = C.pack_weights(w, False, fwd_bf16)
    want_t = C.pack_weights(w, True, dgrad_bf16)
    torch.cuda.synchronize()
    assert pk.dtype == want.dtype and pk.shape == want.shape
    assert pk_t.dtype == want_t.dtype and pk_t.shape == want_t.shape
    assert torch.equal(pk, want)
    assert torch.equal(pk_t, want_t)
