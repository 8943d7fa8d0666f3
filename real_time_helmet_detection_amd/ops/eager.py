"""Eager (plain PyTorch) implementations of the framework ops.

These are the CPU execution path and the numerical oracles for the HIP
kernels: every kernel parity test in tests/ compares the gfx950 kernel
against the fp32 eager op here. On a GPU box the hot path must NOT fall back
to these silently — dispatch in ``ops/__init__`` raises if the HIP extension
is missing for a CUDA tensor.
"""

import functools

import torch
import torch.nn.functional as F


# ---------------------------------------------------------------- losses ---

def centernet_losses(phm, poff, psize, ghm, goff, gsize, mask,
                     focal_alpha, focal_beta, eps=1e-7):
    """Return (hm_focal, offset_l1, size_l1) — math per loss.py docstring."""
    neg_inds = 1.0 - mask
    neg_weights = torch.pow(1.0 - ghm, focal_beta)
    pos_loss = torch.log(phm + eps) * torch.pow(1.0 - phm, focal_alpha) * mask
    neg_loss = (torch.log(1.0 - phm + eps) * torch.pow(phm, focal_alpha)
                * neg_weights * neg_inds)
    num_pos = mask.sum().clamp(1, 1e30)
    hm_loss = -(pos_loss.sum(dim=[1, 2, 3]).mean()
                + neg_loss.sum(dim=[1, 2, 3]).mean()) / num_pos

    off_loss = (poff * mask - goff * mask).abs().sum(dim=[1, 2, 3]).mean() / num_pos
    size_loss = (psize * mask - gsize * mask).abs().sum(dim=[1, 2, 3]).mean() / num_pos
    return hm_loss, off_loss, size_loss


# -------------------------------------------------------- input pipeline ---

def encode_targets(boxes, labels, imsize_hw, scale_factor, num_cls,
                   normalized):
    """Padded (B,N,4) fp32 boxes + (B,N) int32 labels (label < 0 = padding
    row) -> [heatmap, offset, size, mask], by calling transform.box2hm per
    sample on the float32 rows exactly as data.voc collate_fn does."""
    import numpy as np
    from ..transform import box2hm
    H, W = imsize_hw
    boxes_np = boxes.detach().cpu().numpy()
    labels_np = labels.detach().cpu().numpy()
    maps = [[], [], [], []]
    for b, l in zip(boxes_np, labels_np):
        keep = l >= 0
        b, l = b[keep], l[keep]
        out = box2hm(b if len(b) else None, l, (W, H),
                     scale_factor=scale_factor, num_cls=num_cls,
                     normalized=normalized)
        for lst, m in zip(maps, out):
            lst.append(m)
    h, w = H // scale_factor, W // scale_factor
    chans = (num_cls, 2, 2, 1)
    return [torch.from_numpy(np.stack(lst)).to(boxes.device) if lst
            else torch.zeros(0, c, h, w, device=boxes.device)
            for lst, c in zip(maps, chans)]


def normalize_images(img_u8, pretrained, dtype=torch.float32):
    """(B,H,W,3) uint8 -> (B,3,H,W) channels_last, utils.Normalizer applied
    to x.float()/255 (the collate_fn arithmetic), then cast to ``dtype``."""
    from ..utils import get_normalizer
    norm = get_normalizer(pretrained=pretrained)
    x = norm(img_u8.permute(0, 3, 1, 2).float() / 255.0)
    return x.to(dtype).contiguous(memory_format=torch.channels_last)


def _augment_axis(a, b, n, T):
    """One axis of the augment map for outputs 0..T-1 of every image:
    (clamped tap index 0, index 1, in-image mask 0, mask 1, weight), each
    (B, T). a, b fp32 (B,), n int (B,)."""
    i = torch.arange(T, dtype=torch.float32, device=a.device)
    s = a[:, None] * (i + 0.5)[None, :] + b[:, None]
    g = s - 0.5
    nf = n.to(torch.float32)[:, None]
    g = torch.minimum(torch.maximum(g, torch.full_like(g, -2.0)), nf + 1.0)
    g0 = torch.floor(g)
    f = g - g0
    i0 = g0.to(torch.int64)
    i1 = i0 + 1
    n_ = n.to(torch.int64)[:, None]
    m0 = (i0 >= 0) & (i0 < n_)
    m1 = (i1 >= 0) & (i1 < n_)
    zero = torch.zeros_like(i0)
    c0 = torch.minimum(torch.maximum(i0, zero), n_ - 1)
    c1 = torch.minimum(torch.maximum(i1, zero), n_ - 1)
    return c0, c1, m0, m1, f


def augment_images(img_u8, sizes, coef, T, pretrained=None,
                   dtype=torch.float32):
    """Train-time augmentation as one resample (the oracle of
    ops/csrc/augment.hip, tap by tap in the kernel's order so the two can
    be compared bit for bit).

    img_u8 (B,Hmax,Wmax,3) uint8 with image b in its top-left sizes[b] =
    [h, w] corner; coef (B,5) fp32 [ax, bx, ay, by, factor] from
    data.augment.map_coefficients: source = a * output + b per axis in
    continuous coordinates (pixel i centred at i + 0.5). Per output pixel,
    every step rounded to fp32:

        xs = a*(x + 0.5) + b;  g = xs - 0.5;  x0 = floor(g);  fx = g - x0
        tap(p) = in the image ? min(floor(p * factor), 255) : 0
        top = v00*(1-fx) + v01*fx;  bot = v10*(1-fx) + v11*fx
        v = top*(1-fy) + bot*fy;  q = clamp(int(floor(v + 0.5)), 0, 255)

    pretrained=None returns q as (B,T,T,3) uint8; otherwise
    normalize_images(q, pretrained, dtype)."""
    B = img_u8.shape[0]
    T = int(T)
    sizes = sizes.to(img_u8.device)
    coef = coef.to(device=img_u8.device, dtype=torch.float32)
    hmax, wmax = img_u8.shape[1:3]
    h = sizes[:, 0].clamp(1, hmax)
    w = sizes[:, 1].clamp(1, wmax)
    cx0, cx1, mx0, mx1, fx = _augment_axis(coef[:, 0], coef[:, 1], w, T)
    cy0, cy1, my0, my1, fy = _augment_axis(coef[:, 2], coef[:, 3], h, T)
    factor = coef[:, 4].view(B, 1, 1, 1)
    bi = torch.arange(B, device=img_u8.device).view(B, 1, 1)

    def tap(cy, cx, my, mx):
        p = img_u8[bi, cy[:, :, None], cx[:, None, :]].to(torch.float32)
        val = torch.clamp(torch.floor(p * factor), max=255.0)
        mask = (my[:, :, None] & mx[:, None, :]).to(torch.float32)
        return val * mask[..., None]

    fx = fx[:, None, :, None]
    fy = fy[:, :, None, None]
    gx, gy = 1.0 - fx, 1.0 - fy
    top = tap(cy0, cx0, my0, mx0) * gx + tap(cy0, cx1, my0, mx1) * fx
    bot = tap(cy1, cx0, my1, mx0) * gx + tap(cy1, cx1, my1, mx1) * fx
    v = top * gy + bot * fy
    q = torch.floor(v + 0.5).to(torch.int32).clamp(0, 255).to(torch.uint8)
    if pretrained is None:
        return q
    return normalize_images(q, pretrained, dtype)


_RESIZE_PREC = 22  # coefficient precision bits of the 8-bit resample


@functools.lru_cache(maxsize=64)
def _resize_coefficients(n, T):
    """Pillow's 8-bit bilinear coefficients for one axis, n -> T, in float64
    with every operation rounded on its own: (xmin (T,), xmax (T,),
    k (T, K) int64 with zeros past xmax)."""
    f64 = torch.float64
    scale = torch.tensor(float(n), dtype=f64) / torch.tensor(float(T),
                                                             dtype=f64)
    fs = torch.clamp(scale, min=1.0)
    support = fs
    K = int(torch.ceil(support).item()) * 2 + 1
    center = (torch.arange(T, dtype=f64) + 0.5) * scale
    xmin = (center - support + 0.5).to(torch.int64).clamp(min=0)
    xmax = (center + support + 0.5).to(torch.int64).clamp(max=n) - xmin
    x = torch.arange(K, dtype=torch.int64)[None, :]
    t = ((x + xmin[:, None]).to(f64) - center[:, None] + 0.5) / fs
    w = torch.clamp(1.0 - t.abs(), min=0.0)
    w = torch.where(x < xmax[:, None], w, torch.zeros_like(w))
    ww = torch.zeros(T, dtype=f64)
    for j in range(K):  # summed in tap order; a masked tap adds an exact 0
        ww = ww + w[:, j]
    ww = torch.where(ww != 0.0, ww, torch.ones_like(ww))[:, None]
    k = (0.5 + (w / ww) * float(1 << _RESIZE_PREC)).to(torch.int64)
    k = torch.where(x < xmax[:, None], k, torch.zeros_like(k))
    return xmin, xmax, k


def _resize_pass(img, dim, T):
    """One axis of the 8-bit resample: img (h,w,3) uint8 -> size T along
    ``dim`` (0 = vertical, 1 = horizontal), int64 accumulation."""
    n = img.shape[dim]
    xmin, xmax, k = (t.to(img.device) for t in _resize_coefficients(n, T))
    shape = [1, 1, 1]
    shape[dim] = T
    acc = torch.full(shape, 1 << (_RESIZE_PREC - 1), dtype=torch.int64,
                     device=img.device)
    for j in range(int(xmax.max())):
        idx = (xmin + j).clamp(max=n - 1)  # clamped taps have k == 0
        acc = acc + img.index_select(dim, idx).to(torch.int64) \
            * k[:, j].view(shape)
    return (acc >> _RESIZE_PREC).clamp(0, 255).to(torch.uint8)


def check_resize_args(img_u8, sizes, T):
    """Host-side argument checks of resize_images on a CPU copy of
    ``sizes`` (no device sync): every image fits its canvas."""
    hmax, wmax = int(img_u8.shape[1]), int(img_u8.shape[2])
    if int(T) < 1:
        raise ValueError('resize_images: T must be >= 1, got %r' % (T,))
    if sizes.dim() != 2 or tuple(sizes.shape) != (img_u8.shape[0], 2):
        raise ValueError('resize_images: sizes must be (B,2), got %r'
                         % (tuple(sizes.shape),))
    if sizes.numel():
        h, w = sizes[:, 0], sizes[:, 1]
        if int(h.min()) < 1 or int(h.max()) > hmax or int(w.min()) < 1 \
                or int(w.max()) > wmax:
            raise ValueError('resize_images: sizes must satisfy 1 <= h <= '
                             '%d and 1 <= w <= %d' % (hmax, wmax))


def resize_images(img_u8, sizes, T, pretrained=None, dtype=torch.float32):
    """Serving preprocess (the oracle of ops/csrc/preprocess.hip): every
    image of the batch resized to (T, T) exactly as
    PIL.Image.resize((T, T), BILINEAR) does it on 8-bit data.

    img_u8 (B,Hmax,Wmax,3) uint8 with image b in its top-left sizes[b] =
    [h, w] corner (the rest of the canvas is never read). Per axis (input
    size n), in float64:

        scale = n / T;  fs = max(scale, 1);  support = fs
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n) - xmin
        w[x] = max(1 - |x + xmin - center + 0.5| / fs, 0), normalised by
               their sum in tap order;  k[x] = int(0.5 + w[x] * 2^22)
        out = clamp((2^21 + sum_x pixel[xmin + x] * k[x]) >> 22, 0, 255)

    horizontal pass first, rounded to uint8, then the vertical pass over it.

    pretrained=None returns (B,T,T,3) uint8; otherwise
    normalize_images(q, pretrained, dtype)."""
    T = int(T)
    if not sizes.is_cuda:
        check_resize_args(img_u8, sizes, T)
    hmax, wmax = img_u8.shape[1:3]
    out = torch.empty((img_u8.shape[0], T, T, 3), dtype=torch.uint8,
                      device=img_u8.device)
    for b, (h, w) in enumerate(sizes.tolist()):
        h = min(max(int(h), 1), hmax)
        w = min(max(int(w), 1), wmax)
        out[b] = _resize_pass(_resize_pass(img_u8[b, :h, :w], 1, T), 0, T)
    if pretrained is None:
        return out
    return normalize_images(out, pretrained, dtype)


# ---------------------------------------------------------------- conv-ish --

def conv2d(x, weight, bias=None, stride=1, padding=0):
    return F.conv2d(x, weight, bias, stride=stride, padding=padding)


def batch_norm(x, running_mean, running_var, weight, bias, training,
               momentum=0.1, eps=1e-5):
    return F.batch_norm(x, running_mean, running_var, weight, bias,
                        training=training, momentum=momentum, eps=eps)


def conv_bn_act(x, weight, bias, bn, act, stride=1, padding=0, training=False):
    """Fused conv -> BN -> activation (the HIP kernel fuses the epilogue)."""
    y = F.conv2d(x, weight, bias, stride=stride, padding=padding)
    if bn is not None:
        y = F.batch_norm(y, bn.running_mean, bn.running_var, bn.weight,
                         bn.bias, training=training, momentum=bn.momentum,
                         eps=bn.eps)
    return apply_act(y, act)


def apply_act(x, act):
    if act is None or act == 'Linear':
        return x
    if act == 'ReLU':
        return F.relu(x)
    if act == 'LeakyReLU':
        return F.leaky_relu(x, 0.01)
    if act == 'PReLU':
        raise ValueError('PReLU carries parameters; use the module path')
    if act == 'Mish':
        return x * torch.tanh(F.softplus(x))
    if act == 'Sigmoid':
        return torch.sigmoid(x)
    if act == 'CELU':
        return F.celu(x)
    raise ValueError(f'unknown activation {act!r}')


def maxpool2x2(x):
    return F.max_pool2d(x, 2, 2)


def avgpool2x2(x):
    return F.avg_pool2d(x, 2, 2)


def maxpool_same(x, kernel):
    """Stride-1 'same' max pool (SPP branches, peak-NMS)."""
    return F.max_pool2d(x, kernel, stride=1, padding=kernel // 2)


def upsample2x_nearest(x):
    return F.interpolate(x, scale_factor=2, mode='nearest')


# ---------------------------------------------------------------- decode ----

def batched_decode(heatmap, offset, wh, scale_factor, topk, pool_size,
                   normalized):
    """Batched peak-mask + top-k decode.

    heatmap: (B,C,h,w) post-sigmoid; offset/wh: (B,2,h,w).
    Returns (boxes (B,topk,4), classes (B,topk), scores (B,topk)) — no
    confidence filtering (callers threshold), so shapes are static for
    tracing and for the HIP kernel.
    """
    b, c, h, w = heatmap.shape
    hw = h * w
    pad = pool_size // 2
    pooled = F.max_pool2d(heatmap, pool_size, stride=1, padding=pad)
    peakmap = heatmap * (pooled == heatmap)

    scores, indices = peakmap.reshape(b, -1).topk(topk, dim=1)
    clss = torch.div(indices, hw, rounding_mode='floor')
    inds = torch.remainder(indices, hw)
    yinds = torch.div(inds, w, rounding_mode='floor')
    xinds = torch.remainder(inds, w)

    flat_off = offset.reshape(b, 2, hw)
    flat_wh = wh.reshape(b, 2, hw)
    xoffs = flat_off[:, 0].gather(1, inds)
    yoffs = flat_off[:, 1].gather(1, inds)
    xsizs = flat_wh[:, 0].gather(1, inds)
    ysizs = flat_wh[:, 1].gather(1, inds)

    if normalized:
        xoffs = xoffs * scale_factor
        yoffs = yoffs * scale_factor
        xsizs = xsizs * w
        ysizs = ysizs * h

    xc = xinds.to(xoffs.dtype) + xoffs
    yc = yinds.to(yoffs.dtype) + yoffs
    sf = float(scale_factor)
    boxes = torch.stack([(xc - xsizs / 2) * sf, (yc - ysizs / 2) * sf,
                         (xc + xsizs / 2) * sf, (yc + ysizs / 2) * sf], dim=2)
    return boxes, clss, scores


def decode_logits(out, scale_factor, topk, pool_size, normalized,
                  flip=False):
    """Decode the raw network output (Bt,S,C+4,h,w) — the oracle of the
    logits-in kernel (ops/csrc/decode.hip, decode_logits).

    flip=False: sigmoid on the heatmap channels (and on offset/size when
    ``normalized``), then ``batched_decode`` with the stacks as batch.
    flip=True (flip test): item B+b is the output for the horizontally
    mirrored image b, B = Bt/2. In fp32, in this order: p = sigmoid,
    hm = 0.5 * (p(plain) + p(mirrored).flip(-1)), size the same way (p only
    when ``normalized``), offsets from the plain half alone — the mirrored
    image's offsets point the other way (the CenterNet convention).
    Returns (boxes (B*S,topk,4), classes (B*S,topk), scores (B*S,topk)).
    """
    bt, s, k, h, w = out.shape
    c = k - 4
    x = out.float()
    if flip:
        if int(bt) % 2:
            raise ValueError('decode_logits: flip needs an even batch '
                             '(plain half then mirrored half), got %d' % bt)
        b = bt // 2
        x, mirrored = x[:b], x[b:].flip(-1)
    else:
        b = bt
    hm = torch.sigmoid(x[:, :, :c])
    off = x[:, :, c:c + 2]
    wh = x[:, :, c + 2:]
    if normalized:
        off = torch.sigmoid(off)
        wh = torch.sigmoid(wh)
    if flip:
        hm = 0.5 * (hm + torch.sigmoid(mirrored[:, :, :c]))
        wh_m = mirrored[:, :, c + 2:]
        if normalized:
            wh_m = torch.sigmoid(wh_m)
        wh = 0.5 * (wh + wh_m)
    return batched_decode(hm.reshape(b * s, c, h, w),
                          off.reshape(b * s, 2, h, w),
                          wh.reshape(b * s, 2, h, w),
                          scale_factor, topk, pool_size, normalized)


# ------------------------------------------------------------------- nms ----

def box_iou(a, b):
    """IoU matrix between (N,4) and (M,4) xyxy boxes."""
    area_a = (a[:, 2] - a[:, 0]).clamp(min=0) * (a[:, 3] - a[:, 1]).clamp(min=0)
    area_b = (b[:, 2] - b[:, 0]).clamp(min=0) * (b[:, 3] - b[:, 1]).clamp(min=0)
    lt = torch.max(a[:, None, :2], b[None, :, :2])
    rb = torch.min(a[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    union = area_a[:, None] + area_b[None, :] - inter
    return inter / union.clamp(min=1e-9)


def nms(boxes, scores, iou_threshold):
    """Greedy class-agnostic NMS -> kept indices sorted by score.

    Matches torchvision.ops.nms semantics (the reference eval path,
    evaluate.py:174) without depending on torchvision's compiled op.
    """
    n = boxes.shape[0]
    if n == 0:
        return torch.zeros(0, dtype=torch.long, device=boxes.device)
    order = scores.argsort(descending=True)
    boxes_sorted = boxes[order]
    iou = box_iou(boxes_sorted, boxes_sorted)
    keep_mask = torch.ones(n, dtype=torch.bool, device=boxes.device)
    for i in range(n):
        if keep_mask[i]:
            keep_mask[i + 1:] &= iou[i, i + 1:] <= iou_threshold
    return order[keep_mask]


def nms_batched(boxes, scores, iou_threshold, conf_th):
    """Eager twin of the batched NMS kernel: per image, filter by
    conf_th then greedy NMS; returns (idx (B,N) int32 of KEPT original
    indices, counts (B) int32)."""
    B, N = scores.shape
    idx = torch.zeros(B, N, dtype=torch.int32, device=boxes.device)
    counts = torch.zeros(B, dtype=torch.int32, device=boxes.device)
    for i in range(B):
        keep_conf = scores[i] >= conf_th
        sel = keep_conf.nonzero(as_tuple=False).squeeze(1)
        if sel.numel() == 0:
            continue
        kept = nms(boxes[i][sel], scores[i][sel], iou_threshold)
        orig = sel[kept]
        counts[i] = orig.numel()
        idx[i, :orig.numel()] = orig.to(torch.int32)
    return idx, counts


def soft_nms(boxes, scores, iou_threshold=0.3, sigma=0.5, score_th=0.001):
    """Gaussian soft-NMS (reference evaluate.py:184-243 capability).

    Returns (kept_indices, rescored_scores_for_kept) sorted by decayed score.
    """
    n = boxes.shape[0]
    if n == 0:
        return (torch.zeros(0, dtype=torch.long, device=boxes.device),
                torch.zeros(0, device=boxes.device))
    boxes = boxes.float().clone()
    s = scores.float().clone()
    idx = torch.arange(n, device=boxes.device)
    keep = []
    kept_scores = []
    while idx.numel() > 0:
        top = torch.argmax(s[idx])
        cur = idx[top]
        keep.append(cur.item())
        kept_scores.append(s[cur].item())
        rest = torch.cat([idx[:top], idx[top + 1:]])
        if rest.numel() == 0:
            break
        iou = box_iou(boxes[cur][None], boxes[rest])[0]
        s[rest] = s[rest] * torch.exp(-(iou * iou) / sigma)
        idx = rest[s[rest] > score_th]
    device = boxes.device
    return (torch.tensor(keep, dtype=torch.long, device=device),
            torch.tensor(kept_scores, device=device))


def soft_nms_batched(boxes, scores, sigma, score_th, conf_th):
    """Eager twin of the batched soft-NMS kernel: per image, filter by
    conf_th then Gaussian soft-NMS; returns (idx (B,N) int32 original
    indices in selection order, rescored (B,N) float32 decayed scores at
    selection time, counts (B) int32). Entries past counts[b] are 0."""
    B, N = scores.shape
    idx = torch.zeros(B, N, dtype=torch.int32, device=boxes.device)
    out = torch.zeros(B, N, dtype=torch.float32, device=boxes.device)
    counts = torch.zeros(B, dtype=torch.int32, device=boxes.device)
    for i in range(B):
        sel = (scores[i] >= conf_th).nonzero(as_tuple=False).squeeze(1)
        if sel.numel() == 0:
            continue
        kept, rescored = soft_nms(boxes[i][sel], scores[i][sel],
                                  sigma=sigma, score_th=score_th)
        k = kept.numel()
        counts[i] = k
        idx[i, :k] = sel[kept].to(torch.int32)
        out[i, :k] = rescored
    return idx, out, counts


def nms_pack(boxes, classes, scores, box_scale=None, mode=0, iou=0.5,
             sigma=0.5, score_th=0.001, conf=0.0):
    """Eager twin (and oracle) of the packed-emit NMS kernel: either NMS mode
    with a fixed-shape result. boxes (B,N,4), classes (B,N), scores (B,N) ->
    (B, 1+N, 6) float32: row 0 of an image is [count, 0, 0, 0, 0, 0], rows
    1..count are [x1, y1, x2, y2, score, class] in selection order, the rest
    is zero. ``mode`` 0 is ``nms_batched`` (original scores), 1 is
    ``soft_nms_batched`` (rescored scores). ``box_scale`` (4,) or (B,4)
    multiplies the emitted boxes (x, y, x, y)."""
    if mode not in (0, 1):
        raise ValueError('nms_pack: mode 0 (greedy) or 1 (soft), got %r'
                         % (mode,))
    B, N = scores.shape
    boxes = boxes.float()
    scores = scores.float()
    out = torch.zeros(B, 1 + N, 6, dtype=torch.float32, device=boxes.device)
    if N == 0 or B == 0:
        return out
    if mode == 0:
        idx, counts = nms_batched(boxes, scores, iou, conf)
        kept_scores = None
    else:
        idx, kept_scores, counts = soft_nms_batched(boxes, scores, sigma,
                                                    score_th, conf)
    if box_scale is not None:
        box_scale = box_scale.float().reshape(-1, 4).expand(B, 4)
    for i, k in enumerate(counts.tolist()):
        sel = idx[i, :k].long()
        b = boxes[i][sel]
        if box_scale is not None:
            b = b * box_scale[i]
        out[i, 0, 0] = k
        out[i, 1:1 + k, :4] = b
        out[i, 1:1 + k, 4] = scores[i][sel] if kept_scores is None \
            else kept_scores[i, :k]
        out[i, 1:1 + k, 5] = classes[i][sel].float()
    return out


def unpack_detections(packed):
    """A packed (B, 1+N, 6) or single-image (1+N, 6) ``nms_pack`` result, on
    any device -> the per-image lists (boxes (K,4), classes int64 (K),
    scores (K)) that ``postprocess`` returns. One host read of the counts."""
    if packed.dim() == 2:
        packed = packed.unsqueeze(0)
    counts = packed[:, 0, 0].to(torch.int64).cpu().tolist()
    box_lst, cls_lst, score_lst = [], [], []
    for i, k in enumerate(counts):
        rows = packed[i, 1:1 + k]
        box_lst.append(rows[:, :4])
        cls_lst.append(rows[:, 5].to(torch.int64))
        score_lst.append(rows[:, 4])
    return box_lst, cls_lst, score_lst
