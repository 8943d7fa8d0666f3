"""Serving latency with and without flip testing.

python tools/flip_latency.py [--imsize 512] [--batches 1 8] [--iters 200]
    [--rounds 7]

hipGraph-captured bf16 Prediction on the flagship hourglass (1 stack, 128
channels), random weights and inputs (latency does not depend on them):
per batch size one graphed predictor without and one with flip_test, timed
alternately round by round on warm graphs. Wall clock per call including
the NMS host sync, as a caller sees it. Prints one JSON line per batch
size: median and min..max of the rounds in ms, and the ratio of the
medians (the expected cost is that of doubling the network batch).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from real_time_helmet_detection_amd.engine.evaluator import (
    Prediction, GraphedPredictor)
from real_time_helmet_detection_amd.models import StackedHourglass

CL = torch.channels_last


def wall_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--imsize', type=int, default=512)
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 8])
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--in-ch', type=int, default=128)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'flip_latency needs a GPU'

    torch.manual_seed(0)
    net = StackedHourglass(1, args.in_ch, 6).cuda().to(memory_format=CL) \
        .eval()
    for b in args.batches:
        x = torch.randn(b, 3, args.imsize, args.imsize, device='cuda') \
            .contiguous(memory_format=CL)
        preds = {}
        for flip in (False, True):
            p = Prediction(net, topk=100, scale_factor=4, conf_th=0.3,
                           nms='nms', nms_th=0.5, flip_test=flip).cuda()
            preds[flip] = GraphedPredictor(p, x)
        times = {False: [], True: []}
        for flip in (False, True):
            wall_ms(lambda: preds[flip](x), 20)
        for _ in range(args.rounds):
            for flip in (False, True):
                times[flip].append(wall_ms(lambda: preds[flip](x),
                                           args.iters))
        row = {'batch': b, 'imsize': args.imsize, 'dtype': 'bf16',
               'hipgraph': True, 'iters': args.iters, 'rounds': args.rounds}
        for flip, key in ((False, 'plain_ms'), (True, 'flip_ms')):
            t = times[flip]
            row[key] = {'median': round(statistics.median(t), 4),
                        'min': round(min(t), 4), 'max': round(max(t), 4)}
        row['flip_over_plain'] = round(row['flip_ms']['median']
                                       / row['plain_ms']['median'], 3)
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
