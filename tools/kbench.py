"""Micro-benchmark individual HIP kernels (A/B timing + rocprof target).

python tools/kbench.py [wgrad|conv|halo_stats|stem_wgrad|bn|nms|decode|all]
    [--iters N]
    [--variant row|tr|regt]   (wgrad only)
Prints per-kernel ms and effective TFLOP/s on the flagship shapes; ``nms``
prints the hard/soft batched NMS kernels against their eager twins,
``decode`` the logits-in decode against the composition it replaces;
``halo_stats`` the halo conv with its BN-stats epilogue and the one-launch
finish against the conv followed by bn_stats (the table behind
ops.hip._HALO_STATS_MIN_TILES).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from real_time_helmet_detection_amd.ops import _backend

C = _backend.require_ext()
CL = torch.channels_last


def timeit(fn, iters=30, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def bench_wgrad(iters, variant=''):
    # (name, B, cin, cout, hw, k, stride, pad): the first four are the
    # historical table; the rest are the other wgrad shapes of the flagship
    # step (64->128 is the stem-side residual, 152->64 the unfolded stem).
    # The third row was labelled '128->64' until now; its arguments always
    # were cin 64, cout 128, and only the label changed.
    shapes = [
        ('3x3 128ch @128^2 B16', 16, 128, 128, 128, 3, 1, 1),
        ('3x3 128ch @64^2 B16', 16, 128, 128, 64, 3, 1, 1),
        ('3x3 64->128 @256^2 B16', 16, 64, 128, 256, 3, 1, 1),
        ('1x1 128ch @128^2 B16', 16, 128, 128, 128, 1, 1, 0),
        ('1x1 152->64 @256^2 B16', 16, 152, 64, 256, 1, 1, 0),
        ('1x1 128->64 @128^2 B16', 16, 128, 64, 128, 1, 1, 0),
        ('3x3 64ch @128^2 B16', 16, 64, 64, 128, 3, 1, 1),
        ('1x1 128->8 @128^2 B16', 16, 128, 8, 128, 1, 1, 0),
        ('3x3 128ch @32^2 B16', 16, 128, 128, 32, 3, 1, 1),
        ('3x3 128ch @16^2 B16', 16, 128, 128, 16, 3, 1, 1),
        ('3x3 128ch @8^2 B16', 16, 128, 128, 8, 3, 1, 1),
        ('3x3 128ch @256^2 B16', 16, 128, 128, 256, 3, 1, 1),
    ]
    print(f'wgrad variant: {variant or "default dispatch"}')
    for name, B, cin, cout, hw, k, stride, pad in shapes:
        if variant == 'row' and not (k == 3 and stride == 1 and pad == 1
                                     and hw % 32 == 0):
            continue   # the tap-row kernel computes 3x3 s1 p1 only
        x = torch.randn(B, cin, hw, hw, device='cuda',
                        dtype=torch.bfloat16).contiguous(memory_format=CL)
        dy = torch.randn(B, cout, hw, hw, device='cuda',
                         dtype=torch.bfloat16).contiguous(memory_format=CL)
        ms = timeit(lambda: C.wgrad_bf16_fast(x, dy, k, k, stride, pad,
                                              variant=variant), iters)
        fl = 2 * B * hw * hw * cin * cout * k * k
        print(f'wgrad {name:26s} {ms*1e3:8.1f}us  {fl/ms/1e9:7.1f} TF')


def bench_conv(iters):
    shapes = [
        ('3x3 128ch @128^2 B16', 16, 128, 128, 128, 3, 1, 1),
        ('3x3 128ch @256^2 B16', 16, 128, 128, 256, 3, 1, 1),
        ('3x3 128ch @64^2 B16', 16, 128, 128, 64, 3, 1, 1),
        ('3x3 128ch @32^2 B16', 16, 128, 128, 32, 3, 1, 1),
        ('3x3 128ch @16^2 B16', 16, 128, 128, 16, 3, 1, 1),
        ('3x3 128ch @8^2 B16', 16, 128, 128, 8, 3, 1, 1),
        ('1x1 128ch @128^2 B16', 16, 128, 128, 128, 1, 1, 0),
        # the stem-side 3x3 pair of the flagship step (forward and dgrad)
        ('3x3 64->128 @256^2 B16', 16, 64, 128, 256, 3, 1, 1),
        ('3x3 128->64 @256^2 B16', 16, 128, 64, 256, 3, 1, 1),
    ]
    for name, B, cin, cout, hw, k, stride, pad in shapes:
        x = torch.randn(B, cin, hw, hw, device='cuda',
                        dtype=torch.bfloat16).contiguous(memory_format=CL)
        w = torch.randn(cout, cin, k, k, device='cuda') * 0.05
        wpk = C.pack_weights(w, False, True)
        ones = torch.ones(cout, device='cuda')
        zeros = torch.zeros(cout, device='cuda')
        fl = 2 * B * hw * hw * cin * cout * k * k
        # autotuned dispatch (first call measures variants and caches)
        ms = timeit(lambda: C.conv_fwd(x, wpk, ones, zeros, None, k, k,
                                       stride, pad, cout, 1), iters)
        print(f'conv(auto) {name:26s} {ms*1e3:8.1f}us  {fl/ms/1e9:7.1f} TF')
        # explicit variants for the table
        try:
            ms = timeit(lambda: C.conv_fwd_k64(x, wpk, ones, zeros, None,
                                               k, k, stride, pad, cout, 1),
                        iters)
            print(f'conv(k64)  {name:26s} {ms*1e3:8.1f}us  '
                  f'{fl/ms/1e9:7.1f} TF')
        except RuntimeError as e:
            print(f'conv(k64) {name}: {e}')
        if k == 3:
            try:
                ms = timeit(lambda: C.conv_fwd_halo(x, wpk, ones, zeros,
                                                    None, k, k, stride, pad,
                                                    cout, 1), iters)
                print(f'conv(halo) {name:26s} {ms*1e3:8.1f}us  '
                      f'{fl/ms/1e9:7.1f} TF')
            except RuntimeError:
                print(f'conv(halo) {name}: not a multiple of the 8x16 tile')
        for sk in (1, 2, 4, 8, 16):
            if sk > 9 * max(1, cin // 32):
                continue
            try:
                ms = timeit(lambda: C.conv_fwd_small(
                    x, wpk, ones, zeros, None, k, k, stride, pad, cout, 1,
                    sk), iters)
                print(f'conv(64,sk={sk:2d}) {name:22s} {ms*1e3:8.1f}us '
                      f' {fl/ms/1e9:7.1f} TF')
            except RuntimeError as e:
                print(f'conv(64,sk={sk}) {name}: {e}')
                break


def bench_halo_stats(iters, rounds=3):
    """Per 3x3 training-conv shape of the flagship step: the halo conv alone
    (A), with its stats epilogue (B), B + bn_stats_from_parts (C), bn_stats
    alone (D), and the two paths a layer chooses between: C against A + D
    back to back. Medians of `rounds` interleaved rounds, us per call."""
    import statistics
    shapes = [
        ('3x3 64->128 @256^2 B16', 16, 64, 128, 256),
        ('3x3 128ch @256^2 B16', 16, 128, 128, 256),
        ('3x3 128ch @128^2 B16', 16, 128, 128, 128),
        ('3x3 128ch @64^2 B16', 16, 128, 128, 64),
        ('3x3 128ch @32^2 B16', 16, 128, 128, 32),
        ('3x3 128ch @16^2 B16', 16, 128, 128, 16),
    ]
    print('%-24s %6s %8s %8s %8s %8s %9s %7s' % (
        'shape', 'tiles', 'halo', '+stats', '+finish', 'bn_stats',
        'halo+bn', 'saved'))
    for name, B, cin, cout, hw in shapes:
        x = torch.randn(B, cin, hw, hw, device='cuda',
                        dtype=torch.bfloat16).contiguous(memory_format=CL)
        w = torch.randn(cout, cin, 3, 3, device='cuda') * 0.05
        wpk = C.pack_weights(w, False, True)
        ones = torch.ones(cout, device='cuda')
        zeros = torch.zeros(cout, device='cuda')
        rm = torch.zeros(cout, device='cuda')
        rv = torch.ones(cout, device='cuda')
        M = B * hw * hw
        y = C.conv_fwd_halo(x, wpk, ones, zeros, None, 3, 3, 1, 1, cout, 0)

        def halo():
            return C.conv_fwd_halo(x, wpk, ones, zeros, None, 3, 3, 1, 1,
                                   cout, 0)

        def halo_s():
            return C.conv_fwd_halo_stats(x, wpk, ones, zeros, 3, 3, 1, 1,
                                         cout, 0)

        def halo_sf():
            o = halo_s()
            return C.bn_stats_from_parts(o[1], o[2], rm, rv, 0.1, 1e-5, M)

        def stats():
            return C.bn_stats(y, rm, rv, 0.1, 1e-5)

        def halo_bn():
            return C.bn_stats(halo(), rm, rv, 0.1, 1e-5)

        fns = (halo, halo_s, halo_sf, stats, halo_bn)
        t = [[] for _ in fns]
        for fn in fns:
            timeit(fn, 5)
        for _ in range(rounds):
            for i, fn in enumerate(fns):
                t[i].append(timeit(fn, iters, warmup=2) * 1e3)
        m = [statistics.median(v) for v in t]
        tiles = B * (hw // 8) * (hw // 16)
        print('%-24s %6d %8.1f %8.1f %8.1f %8.1f %9.1f %7.1f' % (
            name, tiles, m[0], m[1], m[2], m[3], m[4], m[4] - m[2]))


def bench_fp8(iters):
    shapes = [
        ('3x3 128ch @128^2 B8', 8, 128, 128, 128, 3, 1, 1),
        ('3x3 128ch @256^2 B8', 8, 128, 128, 256, 3, 1, 1),
        # the smallest routed shapes of the b8 and b4 serving steps
        # (M = 32768 and 16384: 256 and 128 blocks)
        ('3x3 128ch @64^2 B8', 8, 128, 128, 64, 3, 1, 1),
        ('3x3 128ch @64^2 B4', 4, 128, 128, 64, 3, 1, 1),
        ('3x3 64->128 @256^2 B8', 8, 64, 128, 256, 3, 1, 1),
        ('1x1 128ch @128^2 B8', 8, 128, 128, 128, 1, 1, 0),
    ]
    for name, B, cin, cout, hw, k, stride, pad in shapes:
        x8 = (torch.randn(B, cin, hw, hw, device='cuda') * 0.5) \
            .to(torch.float8_e4m3fn).contiguous(memory_format=CL)
        w = torch.randn(cout, cin, k, k, device='cuda') * 0.05
        wpk8 = C.pack_weights_fp8(w)
        ones = torch.ones(cout, device='cuda')
        zeros = torch.zeros(cout, device='cuda')
        fl = 2 * B * hw * hw * cin * cout * k * k
        ms = timeit(lambda: C.conv_fwd_fp8r(x8, wpk8, ones, zeros, None,
                                            k, k, stride, pad, cout, 1,
                                            True), iters)
        print(f'conv(fp8 auto) {name:24s} {ms*1e3:8.1f}us  '
              f'{fl/ms/1e9:7.1f} TF')
        if k == 3 and cin == 128:
            # the two kernels conv_fwd_fp8r chooses between: three
            # back-to-back pairs, without and with the e4m3 skip input
            sk8 = (torch.randn(B, cout, hw, hw, device='cuda') * 0.5) \
                .to(torch.float8_e4m3fn).contiguous(memory_format=CL)
            for tag, skip in (('', None), ('+skip', sk8)):
                for _ in range(3):
                    for kind, fn in (('tile128', C.conv_fwd_fp8r_tile128),
                                     ('halo', C.conv_fwd_fp8r_halo)):
                        ms = timeit(lambda: fn(x8, wpk8, ones, zeros, skip,
                                               k, k, stride, pad, cout, 1,
                                               True), iters)
                        label = f'conv(fp8 {kind}{tag})'
                        print(f'{label:24s} {name:22s} {ms*1e3:8.1f}us  '
                              f'{fl/ms/1e9:7.1f} TF')
        # bf16 twin on the same shape for the A/B
        xb = torch.randn(B, cin, hw, hw, device='cuda',
                         dtype=torch.bfloat16).contiguous(memory_format=CL)
        wpk = C.pack_weights(w, False, True)
        ms = timeit(lambda: C.conv_fwd(xb, wpk, ones, zeros, None, k, k,
                                       stride, pad, cout, 1), iters)
        print(f'conv(bf16)     {name:24s} {ms*1e3:8.1f}us  '
              f'{fl/ms/1e9:7.1f} TF')


def bench_stem(iters):
    x = torch.randn(16, 3, 512, 512, device='cuda',
                    dtype=torch.bfloat16).contiguous(memory_format=CL)
    w = torch.randn(64, 3, 7, 7, device='cuda') * 0.05
    ones = torch.ones(64, device='cuda')
    zeros = torch.zeros(64, device='cuda')
    fl = 2 * 16 * 256 * 256 * 64 * 147
    wpk = C.pack_weights(
        torch.nn.functional.pad(
            w.permute(0, 2, 3, 1).reshape(64, -1), (0, 5)
        ).reshape(64, -1, 1, 1), False, True)

    def fwd_path():
        xcol = C.stem_im2col(x, 7, 2, 3)
        return C.conv_fwd(xcol, wpk, ones, zeros, None, 1, 1, 1, 0, 64, 1)
    ms = timeit(fwd_path, iters)
    print(f'stem_fwd(im2col) @512^2 B16   {ms*1e3:8.1f}us  {fl/ms/1e9:7.1f} TF')
    dy = torch.randn(16, 64, 256, 256, device='cuda',
                     dtype=torch.bfloat16).contiguous(memory_format=CL)

    def im2col_path():
        xcol = C.stem_im2col(x, 7, 2, 3)
        return C.wgrad_bf16_fast(xcol, dy, 1, 1, 1, 0)
    ms = timeit(im2col_path, iters)
    print(f'stem_wgrad(im2col) @512^2 B16 {ms*1e3:8.1f}us  {fl/ms/1e9:7.1f} TF')


def bench_bn(iters):
    x = torch.randn(16, 128, 128, 128, device='cuda',
                    dtype=torch.bfloat16).contiguous(memory_format=CL)
    gb = torch.ones(128, device='cuda')
    bt = torch.zeros(128, device='cuda')
    mean, rstd = C.bn_stats(x, None, None, 0.1, 1e-5)
    nbytes = x.numel() * 2
    ms = timeit(lambda: C.bn_stats(x, None, None, 0.1, 1e-5), iters)
    print(f'bn_stats 128ch@128^2 B16      {ms*1e3:8.1f}us  {nbytes/ms/1e9:7.1f} GB/s')
    ms = timeit(lambda: C.bn_act_fwd(x, mean, rstd, gb, bt, 1), iters)
    print(f'bn_act_fwd                    {ms*1e3:8.1f}us  {2*nbytes/ms/1e9:7.1f} GB/s')
    dy = torch.randn_like(x)
    ms = timeit(lambda: C.bn_act_bwd(dy, x, mean, rstd, gb, bt, 1), iters)
    print(f'bn_act_bwd (all 3 kernels)    {ms*1e3:8.1f}us  {5*nbytes/ms/1e9:7.1f} GB/s')


def clustered_boxes(b, n, seed):
    """Seeded detector-like candidates: 8 cluster centres in a 512^2 frame,
    centre + N(0,10), sides 40-80 px, scores U(0.05, 1)."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.rand(b, 8, 2, generator=g) * 512
    which = torch.randint(0, 8, (b, n), generator=g)
    c = torch.gather(centres, 1, which[..., None].expand(b, n, 2)) \
        + torch.randn(b, n, 2, generator=g) * 10
    wh = 40 + 40 * torch.rand(b, n, 2, generator=g)
    boxes = torch.cat([c - wh / 2, c + wh / 2], dim=2)
    scores = 0.05 + 0.95 * torch.rand(b, n, generator=g)
    return boxes.cuda(), scores.cuda()


def wall_ms(fn, iters, warmup=2):
    """Wall clock per call; fn ends with the host sync its caller pays."""
    import time
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def bench_nms(iters):
    """Hard and soft batched NMS incl. the counts.cpu() sync, HIP kernel vs
    the eager twin on the same GPU tensors (what RTHD_EAGER_GPU=1 runs)."""
    from real_time_helmet_detection_amd.ops import eager, hip
    conf = 0.3
    print('batched NMS + counts.cpu(), conf_th %.1f, wall us per call' % conf)
    print('%-5s %2s %4s %5s %10s %10s %8s'
          % ('mode', 'B', 'N', 'kept', 'kernel', 'eager', 'ratio'))
    for b in (1, 8):
        for n in (100, 400):
            boxes, scores = clustered_boxes(b, n, seed=b * 1000 + n)
            runs = (
                ('hard',
                 lambda: hip.nms_batched(boxes, scores, 0.5, conf)[-1].cpu(),
                 lambda: eager.nms_batched(boxes, scores, 0.5,
                                           conf)[-1].cpu()),
                ('soft',
                 lambda: hip.soft_nms_batched(boxes, scores, 0.5, conf,
                                              conf)[-1].cpu(),
                 lambda: eager.soft_nms_batched(boxes, scores, 0.5, conf,
                                                conf)[-1].cpu()),
            )
            for mode, kern, eag in runs:
                kept = int(kern().sum())
                k_ms = wall_ms(kern, iters)
                e_ms = wall_ms(eag, max(2, iters // 10), warmup=1)
                print('%-5s %2d %4d %5d %10.1f %10.1f %7.1fx'
                      % (mode, b, n, kept, k_ms * 1e3, e_ms * 1e3,
                         e_ms / k_ms))


def decode_composition(out, flip, topk):
    """What decode_logits replaces, from existing ops only: upcast, split,
    sigmoid, (flip, add, scale), then the maps-in decode_fwd."""
    bt, s, k, h, w = out.shape
    flat = out.reshape(bt * s, k, h, w).float()
    hm, off, wh = flat.split([k - 4, 2, 2], dim=1)
    hm = torch.sigmoid(hm)
    if flip:
        n = bt * s // 2
        hm = 0.5 * (hm[:n] + hm[n:].flip(-1))
        wh = 0.5 * (wh[:n] + wh[n:].flip(-1))
        off = off[:n]
    return C.decode_fwd(hm, off, wh, 4, topk, 3, False)


def bench_decode(iters, rounds=9):
    """decode_logits against decode_composition on bf16 logits
    (Bt,1,6,128,128), images B of 1 and 8, flip off and on. A and B
    alternate round by round on warm kernels; prints the median and the
    min..max of the rounds (us per call, device time) and the ratio of
    the medians."""
    import statistics
    topk = 100
    print('decode: fused decode_logits (A) vs composition + decode_fwd (B),'
          ' bf16 (Bt,1,6,128,128), topk %d, %d rounds x %d calls'
          % (topk, rounds, iters))
    print('%2s %5s %30s %30s %7s'
          % ('B', 'flip', 'A us med (min..max)', 'B us med (min..max)',
             'B/A'))
    for b in (1, 8):
        for flip in (False, True):
            bt = 2 * b if flip else b
            g = torch.Generator().manual_seed(100 * b + flip)
            out = (torch.randn(bt, 1, 6, 128, 128, generator=g) * 2 - 2) \
                .to(torch.bfloat16).cuda()
            fa = lambda: C.decode_logits(out, 4, topk, 3, False, flip)  # noqa
            fb = lambda: decode_composition(out, flip, topk)  # noqa
            ta, tb = [], []
            timeit(fa, iters)
            timeit(fb, iters)
            for _ in range(rounds):
                ta.append(timeit(fa, iters, warmup=2) * 1e3)
                tb.append(timeit(fb, iters, warmup=2) * 1e3)
            ma, mb = statistics.median(ta), statistics.median(tb)
            print('%2d %5s %12.1f (%6.1f..%6.1f) %14.1f (%6.1f..%6.1f) %6.2fx'
                  % (b, flip, ma, min(ta), max(ta), mb, min(tb), max(tb),
                     mb / ma))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('which', nargs='?', default='all')
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--variant', default='',
                    choices=['', 'row', 'tr', 'regt'],
                    help='wgrad kernel: row = tap-row, tr = transposed-read, '
                         'regt = register-transpose; default = the host dispatch '
                         'rule')
    args = ap.parse_args()
    torch.manual_seed(0)
    if args.which in ('wgrad', 'all'):
        bench_wgrad(args.iters, args.variant)
    if args.which in ('conv', 'all'):
        bench_conv(args.iters)
    if args.which in ('halo_stats', 'all'):
        bench_halo_stats(args.iters)
    if args.which in ('fp8', 'all'):
        bench_fp8(args.iters)
    if args.which in ('stem', 'stem_wgrad', 'all'):
        bench_stem(args.iters)
    if args.which in ('bn', 'all'):
        bench_bn(args.iters)
    if args.which in ('nms', 'all'):
        bench_nms(args.iters)
    if args.which in ('decode', 'all'):
        bench_decode(args.iters)
