"""TorchScript export path (parity with /root/reference/export.py:8-152).

``Export`` is the trace-friendly predictor variant: fixed batch=1, static
top-k decode, and a @torch.jit.script greedy NMS (loops preserved
symbolically, not trace-unrolled) so the traced module is self-contained —
the C++ inference app (tools/cpp_infer) loads it with LibTorch and needs no
python. ``export_model`` traces and saves the cpu/gpu variants
(jit_traced_model_cpu.pth / jit_traced_model_gpu.pth, export.py:120-130).
``RawExport`` puts the device preprocess in front of it; ``ServeExport`` is
the serving form: raw frame in, one packed fixed-shape detection tensor out
(rthd::nms_pack), nothing inside that needs the host, so the consumer can
replay it from a captured graph.
"""

from typing import Tuple

import torch

from ..ops import _backend
from ..transform import hm2box


@torch.jit.script
def nms_scripted(boxes: torch.Tensor, scores: torch.Tensor,
                 threshold: float) -> torch.Tensor:
    """Greedy IoU suppression, scripted so the loop survives tracing."""
    order = torch.argsort(scores, descending=True)
    b = boxes[order]
    s = scores[order].clone()
    n = b.shape[0]
    area = (b[:, 2] - b[:, 0]).clamp(min=0.) * (b[:, 3] - b[:, 1]).clamp(min=0.)
    for i in range(n - 1):
        if float(s[i]) == 0.:
            continue
        xx1 = torch.max(b[i, 0], b[i + 1:, 0])
        yy1 = torch.max(b[i, 1], b[i + 1:, 1])
        xx2 = torch.min(b[i, 2], b[i + 1:, 2])
        yy2 = torch.min(b[i, 3], b[i + 1:, 3])
        w = (xx2 - xx1).clamp(min=0.)
        h = (yy2 - yy1).clamp(min=0.)
        inter = w * h
        iou = inter / (area[i] + area[i + 1:] - inter).clamp(min=1e-9)
        s[i + 1:] = s[i + 1:] * (iou < threshold).to(s.dtype)
    return order[s > 0]


@torch.jit.script
def soft_nms_scripted(boxes: torch.Tensor, scores: torch.Tensor,
                      sigma: float, score_th: float
                      ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Gaussian soft-NMS with ops.eager.soft_nms semantics, scripted so the
    data-dependent loop survives tracing. Returns (kept indices in
    selection order, decayed scores at selection time)."""
    n = boxes.shape[0]
    b = boxes.float()
    s = scores.float().clone()
    area = (b[:, 2] - b[:, 0]).clamp(min=0.) * (b[:, 3] - b[:, 1]).clamp(min=0.)
    # round 1 selects unconditionally; afterwards only scores > score_th live
    alive = torch.ones(n, dtype=torch.bool, device=boxes.device)
    keep = torch.zeros(n, dtype=torch.long, device=boxes.device)
    kept = torch.zeros(n, dtype=torch.float32, device=boxes.device)
    neg = torch.full_like(s, float('-inf'))
    k = 0
    while bool(alive.any()):
        cur = torch.argmax(torch.where(alive, s, neg))
        keep[k] = cur
        kept[k] = s[cur]
        k += 1
        alive[cur] = False
        xx1 = torch.max(b[cur, 0], b[:, 0])
        yy1 = torch.max(b[cur, 1], b[:, 1])
        xx2 = torch.min(b[cur, 2], b[:, 2])
        yy2 = torch.min(b[cur, 3], b[:, 3])
        inter = (xx2 - xx1).clamp(min=0.) * (yy2 - yy1).clamp(min=0.)
        iou = inter / (area[cur] + area - inter).clamp(min=1e-9)
        s = torch.where(alive, s * torch.exp(-(iou * iou) / sigma), s)
        alive = alive & (s > score_th)
    return keep[:k], kept[:k]


NMS_MODES = ('nms', 'soft-nms')


class Export(torch.nn.Module):
    """Traceable single-image predictor: net -> sigmoid -> decode -> NMS.

    Unlike the reference (which hardcoded split([2,2,2]) i.e. num_cls=2,
    export.py:31) the class count is taken from the constructor.
    Returns (boxes, classes, scores) for the first batch item. ``nms``
    selects 'nms' (greedy IoU) or 'soft-nms' (Gaussian, sigma 0.5, drop at
    conf_th like ``Prediction``; returns the rescored scores).
    ``flip_test`` runs the network on the image and its horizontal mirror
    as a batch of two and decodes their merged maps once (``_forward_flip``);
    input and outputs stay those of the one image.
    """

    def __init__(self, network, topk, scale_factor, conf_th, nms_th,
                 normalized_coord=False, num_cls=2, pool_size=3, nms='nms',
                 flip_test=False):
        super().__init__()
        if nms not in NMS_MODES:
            raise NotImplementedError(
                'Not expected nms algorithm: %s' % nms)
        self.nms = nms
        self.flip_test = flip_test
        self.network = network
        self.topk = topk
        self.scale_factor = scale_factor
        self.conf_th = conf_th
        self.nms_th = nms_th
        self.normalized_coord = normalized_coord
        self.num_cls = num_cls
        self.pool_size = pool_size

    def forward(self, x):
        if self.flip_test:
            return self._forward_flip(x)
        batch_output = self.network(x)  # (1, S, num_cls+4, h, w)
        outputs = batch_output[0]  # (S, num_cls+4, h, w)
        if outputs.is_cuda and not _backend.eager_gpu_override():
            return self._forward_native(outputs)
        stack_boxes = []
        stack_clss = []
        stack_scores = []
        for output in outputs.split(1, dim=0):
            out = output.squeeze(0).float()
            heatmap, offset, wh = out.split([self.num_cls, 2, 2], dim=0)
            heatmap = torch.sigmoid(heatmap)
            if self.normalized_coord:
                offset = torch.sigmoid(offset)
                wh = torch.sigmoid(wh)
            boxes, clss, scores = hm2box(
                heatmap=heatmap, offset=offset, wh=wh,
                scale_factor=self.scale_factor, topk=self.topk,
                conf_th=self.conf_th, normalized=self.normalized_coord,
                pool_size=self.pool_size)
            stack_boxes.append(boxes)
            stack_clss.append(clss)
            stack_scores.append(scores)
        boxes = torch.cat(stack_boxes, dim=0)
        clss = torch.cat(stack_clss, dim=0)
        scores = torch.cat(stack_scores, dim=0)
        if self.nms == 'soft-nms':
            keep, rescored = soft_nms_scripted(boxes, scores, 0.5,
                                               float(self.conf_th))
            return boxes[keep], clss[keep], rescored
        keep = nms_scripted(boxes, scores, self.nms_th)
        return boxes[keep], clss[keep], scores[keep]

    def _forward_native(self, outputs):
        """GPU decode: stacks-as-batch through the fused peak+topk decode
        kernel and the LDS-resident NMS — 3 kernels instead of ~25 small
        ops per stack plus a scripted NMS loop whose float(s[i]) costs one
        device sync per candidate (the eager export ran at 65 FPS in the
        C++ app; this path at 150+)."""
        return self._nms_native(*self._decode_plain(outputs))

    def _decode_plain(self, outputs):
        """(S, num_cls+4, h, w) network output of the one image -> the
        decode kernel's (boxes (S,topk,4), classes, scores)."""
        outs = outputs.float()  # (S, num_cls+4, h, w)
        heatmap, offset, wh = outs.split([self.num_cls, 2, 2], dim=1)
        heatmap = torch.sigmoid(heatmap)
        if self.normalized_coord:
            offset = torch.sigmoid(offset)
            wh = torch.sigmoid(wh)
        return torch.ops.rthd.decode(
            heatmap, offset, wh, self.scale_factor, self.topk,
            self.pool_size, self.normalized_coord)

    def _decode_flip(self, out):
        """(2, S, num_cls+4, h, w) output of image and mirror -> the merged
        logits-in decode."""
        if out.dtype != torch.bfloat16:
            out = out.float()
        return torch.ops.rthd.decode_logits(
            out.contiguous(), self.scale_factor, self.topk,
            self.pool_size, self.normalized_coord, True)

    def decode_native(self, x):
        """Network and native GPU decode of this configuration (plain or
        flip test), without the NMS: what ``forward`` feeds ``_nms_native``
        and ``ServeExport`` feeds the packed NMS."""
        if self.flip_test:
            return self._decode_flip(
                self.network(torch.cat([x[:1], x[:1].flip(3)])))
        return self._decode_plain(self.network(x)[0])

    def _nms_native(self, b, c, s):
        boxes = b.reshape(-1, 4)
        clss = c.reshape(-1)
        scores = s.reshape(-1)
        keep = scores >= self.conf_th
        boxes, clss, scores = boxes[keep], clss[keep], scores[keep]
        if self.nms == 'soft-nms':
            keep, rescored = torch.ops.rthd.soft_nms(
                boxes, scores, 0.5, float(self.conf_th))
            return boxes[keep], clss[keep], rescored
        keep = torch.ops.rthd.nms(boxes, scores, float(self.nms_th))
        return boxes[keep], clss[keep], scores[keep]

    def _forward_flip(self, x):
        """Flip test on the one input image: the network runs on a batch of
        two (image, horizontal mirror) and the logits-in decode merges the
        halves. GPU: rthd::decode_logits and the native NMS; CPU (or the
        eager override): the eager composition and the scripted NMS."""
        from ..ops import eager
        out = self.network(torch.cat([x[:1], x[:1].flip(3)]))
        if out.is_cuda and not _backend.eager_gpu_override():
            return self._nms_native(*self._decode_flip(out))
        b, c, s = eager.decode_logits(
            out, self.scale_factor, self.topk, self.pool_size,
            self.normalized_coord, flip=True)
        boxes = b.reshape(-1, 4)
        clss = c.reshape(-1)
        scores = s.reshape(-1)
        keep = scores >= self.conf_th
        boxes, clss, scores = boxes[keep], clss[keep], scores[keep]
        if self.nms == 'soft-nms':
            keep, rescored = soft_nms_scripted(boxes, scores, 0.5,
                                               float(self.conf_th))
            return boxes[keep], clss[keep], rescored
        keep = nms_scripted(boxes, scores, self.nms_th)
        return boxes[keep], clss[keep], scores[keep]


class RawExport(torch.nn.Module):
    """Raw-frame front end of ``Export`` for the GPU-native trace: one
    (H,W,3) uint8 device frame of any size -> rthd::resize_frame (the
    Pillow-exact resize to ``imsize`` and the normalise, one pass on the
    device) -> ``Export`` -> (boxes in the frame's own pixels, classes,
    scores). The op reads H and W from the tensor when it runs, so a trace
    holds nothing about the example frame's size."""

    def __init__(self, export, imsize, pretrained='imagenet'):
        super().__init__()
        from ..ops import hip
        self.export = export
        self.imsize = int(imsize)
        self.register_buffer(
            'table', hip._norm_table(torch.device('cuda',
                                                  torch.cuda.current_device()),
                                     pretrained, torch.float32).clone())

    def forward(self, frame):
        image, scale = torch.ops.rthd.resize_frame(frame, self.imsize,
                                                   self.table)
        boxes, clss, scores = self.export(image)
        return boxes * scale, clss, scores


SERVE_CAP = 2048  # candidates per image of the packed NMS (nms_common.h)


class ServeExport(torch.nn.Module):
    """The serving trace: one (H,W,3) uint8 device frame of any size ->
    rthd::resize_frame -> network -> the decode of ``export`` (plain or flip
    test) -> rthd::nms_pack with the confidence filter, the NMS mode and the
    box rescale folded in -> ONE (1+N, 6) float32 tensor, N = stacks * topk:
    row 0 is [count, 0, 0, 0, 0, 0], rows 1..count are [x1, y1, x2, y2,
    score, class] in the frame's own pixels, the rest is zero.

    Every op has a shape fixed by the configuration and none reads back to
    the host, so a consumer may capture the whole forward into a graph
    (tools/cpp_infer ``-g``, tools/serve_latency.py) and fetch the result
    with one copy."""

    def __init__(self, export, imsize, pretrained='imagenet'):
        super().__init__()
        from ..ops import hip
        self.export = export
        self.imsize = int(imsize)
        self.mode = NMS_MODES.index(export.nms)
        self.register_buffer(
            'table', hip._norm_table(torch.device('cuda',
                                                  torch.cuda.current_device()),
                                     pretrained, torch.float32).clone())

    def forward(self, frame):
        image, scale = torch.ops.rthd.resize_frame(frame, self.imsize,
                                                   self.table)
        b, c, s = self.export.decode_native(image)
        n = b.shape[0] * b.shape[1]
        if n > SERVE_CAP:
            raise ValueError(
                'serving export: num_stack * topk = %d candidates exceed '
                'the packed NMS limit of %d' % (n, SERVE_CAP))
        e = self.export
        # soft mode: sigma 0.5, drop at conf_th, as Export and Prediction
        packed = torch.ops.rthd.nms_pack(
            b.reshape(1, n, 4), c.reshape(1, n), s.reshape(1, n), scale,
            self.mode, float(e.nms_th), 0.5, float(e.conf_th),
            float(e.conf_th))
        return packed[0]


def build_serve_module(args, network, imsize):
    """``ServeExport`` over ``build_export_module`` for the parsed flags."""
    n = args.num_stack * args.topk
    if n > SERVE_CAP:
        raise ValueError(
            '--serve: --num-stack * --topk = %d candidates exceed the packed '
            'NMS limit of %d; lower --topk' % (n, SERVE_CAP))
    if not torch.cuda.is_available():
        raise RuntimeError('--serve needs a GPU and the kernel extension')
    _backend.require_ext()
    return ServeExport(build_export_module(args, network), imsize,
                       args.pretrained)


def build_export_module(args, network):
    return Export(
        network=network, topk=args.topk, scale_factor=args.scale_factor,
        conf_th=args.conf_th, nms_th=args.nms_th,
        normalized_coord=args.normalized_coord, num_cls=args.num_cls,
        pool_size=args.pool_size, nms=args.nms,
        flip_test=getattr(args, 'flip_test', False))


def _trace_contexts(infer_dtype):
    """The contexts a GPU trace of ``infer_dtype`` runs under: the amp
    contexts of --infer-dtype, with torch.autocast's weight cache off (the
    tracer must see every cast autocast inserts as an explicit op of this
    trace, not a tensor cached by the warm-up call)."""
    import contextlib
    from .. import amp
    stack = contextlib.ExitStack()
    stack.enter_context(amp.infer_context(infer_dtype))
    if infer_dtype != 'fp32':
        stack.enter_context(torch.autocast(
            device_type='cuda', dtype=torch.bfloat16, cache_enabled=False))
    return stack


def export_model(predictor, save_dir='.', imsize=512, do_gpu=None,
                 native=True, raw_input=False, pretrained='imagenet',
                 infer_dtype='fp32', serve=None):
    """Trace and save cpu (and, if available, gpu) TorchScript models.

    The CPU trace records plain torch-ROCm eager ops — self-contained and
    loadable by any LibTorch (the reference's portability property,
    export.py:120-130). The GPU trace records the NATIVE gfx950 kernels via
    their dispatcher registrations (torch.ops.rthd.*, TORCH_LIBRARY in
    ops/csrc/bindings.cpp) — packed weights and folded BN scales are baked
    into the graph as constants; the consumer (tools/cpp_infer, ``-k``)
    dlopens the kernel extension before loading. Pass ``native=False`` (or
    set RTHD_EXPORT_EAGER=1) for a portable eager-op GPU trace instead.

    ``raw_input`` additionally saves jit_traced_model_gpu_raw.pth, the
    native GPU trace behind ``RawExport``: it takes the raw uint8 frame and
    normalises with the ``pretrained`` scheme. The other files are the same
    with and without it.

    ``infer_dtype`` 'bf16' / 'fp8' traces every GPU file under
    ``amp.autocast`` (plus ``amp.fp8_autocast``) and saves it with a
    ``_bf16`` / ``_fp8`` suffix before ``.pth``, next to (never over) an
    fp32 export; the bf16 / e4m3 packed weights and the casts are part of
    the trace, so the consumer needs no autocast state. The CPU trace is
    always fp32. ``serve`` (a ``ServeExport``) additionally saves
    jit_traced_model_gpu_serve<suffix>.pth.
    """
    import os
    from ..config import INFER_DTYPES
    if infer_dtype not in INFER_DTYPES:
        raise ValueError('infer_dtype must be one of %s, got %r'
                         % (', '.join(INFER_DTYPES), infer_dtype))
    os.makedirs(save_dir, exist_ok=True)
    predictor.eval()
    paths = {}

    x = torch.randn(1, 3, imsize, imsize)
    with torch.no_grad():
        traced_cpu = torch.jit.trace(predictor.cpu(), x)
    p = os.path.join(save_dir, 'jit_traced_model_cpu.pth')
    torch.jit.save(traced_cpu, p)
    paths['cpu'] = p
    print('Model saved at cpu:', p)

    if do_gpu is None:
        do_gpu = torch.cuda.is_available()
    if not do_gpu and (infer_dtype != 'fp32' or serve is not None):
        raise RuntimeError('infer_dtype %s / the serving export need a GPU'
                           % infer_dtype)
    if do_gpu:
        if os.environ.get('RTHD_EXPORT_EAGER'):
            native = False
        if not native and (infer_dtype != 'fp32' or serve is not None):
            raise RuntimeError('bf16 / fp8 and the serving export record '
                               'the native rthd ops: no eager variant')
        suffix = '' if infer_dtype == 'fp32' else '_' + infer_dtype
        prev = os.environ.get('RTHD_EAGER_GPU')
        if not native:
            os.environ['RTHD_EAGER_GPU'] = '1'
        try:
            xg = torch.randn(1, 3, imsize, imsize, device='cuda')
            predictor = predictor.cuda()
            with torch.no_grad(), _trace_contexts(infer_dtype):
                if native:
                    # warm the conv inference caches first: the trace then
                    # bakes the FROZEN packed-weight/scale/shift tensors as
                    # constants (exact replay); a cold-cache trace records
                    # the fold chain and was measured to misreplay. Under
                    # the same contexts, so the frozen tensors are those of
                    # infer_dtype.
                    predictor(xg)
                traced_gpu = torch.jit.trace(predictor, xg)
            p = os.path.join(save_dir, 'jit_traced_model_gpu%s.pth' % suffix)
            torch.jit.save(traced_gpu, p)
            paths['gpu'] = p
            print('Model saved at gpu (%s ops): %s'
                  % ('native rthd' if native else 'eager', p))
            if raw_input:
                if not native:
                    raise RuntimeError('the raw-input export records the '
                                       'native rthd ops: no eager variant')
                raw = RawExport(predictor, imsize, pretrained).cuda().eval()
                frame = torch.randint(0, 256, (imsize, imsize, 3),
                                      dtype=torch.uint8, device='cuda')
                with torch.no_grad(), _trace_contexts(infer_dtype):
                    traced_raw = torch.jit.trace(raw, frame)
                p = os.path.join(save_dir,
                                 'jit_traced_model_gpu_raw%s.pth' % suffix)
                torch.jit.save(traced_raw, p)
                paths['gpu_raw'] = p
                print('Raw-input model saved at gpu: %s (takes a (H,W,3) '
                      'uint8 frame; needs the kernel extension to load)' % p)
            if serve is not None:
                serve = serve.cuda().eval()
                frame = torch.randint(0, 256, (imsize, imsize, 3),
                                      dtype=torch.uint8, device='cuda')
                with torch.no_grad(), _trace_contexts(infer_dtype):
                    # its Export may be another module than ``predictor``
                    # (or run the flip-test batch of two): warm it as well
                    serve(frame)
                    traced_serve = torch.jit.trace(serve, frame)
                p = os.path.join(save_dir,
                                 'jit_traced_model_gpu_serve%s.pth' % suffix)
                torch.jit.save(traced_serve, p)
                paths['gpu_serve'] = p
                print('Serving model saved at gpu: %s (takes a (H,W,3) '
                      'uint8 frame, returns packed (1+N, 6) detections; '
                      'needs the kernel extension to load)' % p)
        finally:
            if prev is None:
                os.environ.pop('RTHD_EAGER_GPU', None)
            else:
                os.environ['RTHD_EAGER_GPU'] = prev
    return paths
