"""Latency of a serving trace: plain calls against graph replay.

python tools/serve_latency.py --model jit_traced_model_gpu_serve_bf16.pth
    [--frame 1080 1920] [--iters 200] [--rounds 7]

Loads a serving trace (export.py --serve; the kernel extension is imported
first so the rthd:: ops resolve), feeds it one random uint8 frame (latency
does not depend on the pixels), captures one forward with torch.cuda.graph
after three warm-up calls on a side stream, and times plain calls and
replays alternately round by round. Each timed call uploads the frame from
pinned host memory into the static input and ends with the packed tensor in
pinned host memory (one copy each way and a synchronise), as a consumer sees
it. Before timing, the replay is compared with the plain call
(equal). Prints one JSON line: median and min..max of the rounds in ms, and
the ratio of the medians.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from real_time_helmet_detection_amd.ops import _backend


def wall_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', required=True)
    ap.add_argument('--frame', type=int, nargs=2, default=[1080, 1920],
                    metavar=('H', 'W'))
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'serve_latency needs a GPU'
    _backend.require_ext()

    model = torch.jit.load(args.model).cuda().eval()
    g = torch.Generator().manual_seed(0)
    host_in = torch.randint(0, 256, (*args.frame, 3), dtype=torch.uint8,
                            generator=g).pin_memory()
    static_in = host_in.cuda()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(3):
            want = model(static_in)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        static_out = model(static_in)
    host_out = torch.empty(static_out.shape, dtype=static_out.dtype,
                           pin_memory=True)

    @torch.no_grad()
    def plain():
        static_in.copy_(host_in, non_blocking=True)
        host_out.copy_(model(static_in), non_blocking=True)
        torch.cuda.synchronize()

    def replay():
        static_in.copy_(host_in, non_blocking=True)
        graph.replay()
        host_out.copy_(static_out, non_blocking=True)
        torch.cuda.synchronize()

    replay()
    assert torch.equal(host_out, want.cpu()), 'replay differs from plain call'
    fns = {'plain_ms': plain, 'graph_ms': replay}
    times = {k: [] for k in fns}
    for fn in fns.values():
        wall_ms(fn, 20)
    for _ in range(args.rounds):
        for key, fn in fns.items():
            times[key].append(wall_ms(fn, args.iters))
    row = {'model': os.path.basename(args.model), 'frame': args.frame,
           'detections': int(host_out[0, 0]), 'iters': args.iters,
           'rounds': args.rounds}
    for key, t in times.items():
        row[key] = {'median': round(statistics.median(t), 4),
                    'min': round(min(t), 4), 'max': round(max(t), 4)}
    row['plain_over_graph'] = round(row['plain_ms']['median']
                                    / row['graph_ms']['median'], 3)
    print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
