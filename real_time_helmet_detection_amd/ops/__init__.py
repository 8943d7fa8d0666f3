"""Op dispatch layer.

Every hot op of the detector goes through this module:

- CPU tensors -> ``eager`` (plain PyTorch; also the test oracle).
- CUDA(ROCm) tensors -> ``hip`` (hand-written gfx950 kernels from the in-tree
  extension). A missing extension is a hard error, never a silent fallback.
- ``RTHD_EAGER_GPU=1`` forces eager on GPU for explicit A/B measurement only.

Replaces, MI355X-natively, what the reference delegated to cuDNN/torchvision
(SURVEY.md §2.3): fused conv+BN+act, pooling, upsample, the fused
focal+L1 loss, the maxpool-peak top-k decode, NMS and Gaussian soft-NMS
(both NMS modes are batched kernels: one launch and one host sync per
batch).
"""

import torch

from . import eager
from . import _backend


def _hip(x):
    return x.is_cuda and not _backend.eager_gpu_override()


# ---------------------------------------------------------------- losses ---

def centernet_losses(phm, poff, psize, ghm, goff, gsize, mask,
                     focal_alpha, focal_beta):
    if _hip(phm):
        from . import hip
        return hip.centernet_losses(phm, poff, psize, ghm, goff, gsize, mask,
                                    focal_alpha, focal_beta)
    return eager.centernet_losses(phm, poff, psize, ghm, goff, gsize, mask,
                                  focal_alpha, focal_beta)


# ---------------------------------------------------------------- decode ---

def batched_decode(heatmap, offset, wh, scale_factor, topk, pool_size,
                   normalized):
    if _hip(heatmap):
        from . import hip
        return hip.batched_decode(heatmap, offset, wh, scale_factor, topk,
                                  pool_size, normalized)
    return eager.batched_decode(heatmap, offset, wh, scale_factor, topk,
                                pool_size, normalized)


def decode_logits(out, scale_factor, topk, pool_size, normalized,
                  flip=False):
    # raw (Bt,S,C+4,h,w) network output in; flip=True merges the mirrored
    # half B..2B-1 into the plain half (flip test)
    if _hip(out):
        from . import hip
        return hip.decode_logits(out, scale_factor, topk, pool_size,
                                 normalized, flip)
    return eager.decode_logits(out, scale_factor, topk, pool_size,
                               normalized, flip)


def nms(boxes, scores, iou_threshold):
    if _hip(boxes):
        from . import hip
        return hip.nms(boxes, scores, iou_threshold)
    return eager.nms(boxes, scores, iou_threshold)


def nms_batched(boxes, scores, iou_threshold, conf_th):
    if _hip(boxes):
        from . import hip
        return hip.nms_batched(boxes, scores, iou_threshold, conf_th)
    return eager.nms_batched(boxes, scores, iou_threshold, conf_th)


def soft_nms(boxes, scores, iou_threshold=0.3, sigma=0.5, score_th=0.001):
    # serial argmax+decay rounds: one wave per image on GPU (soft_nms.hip);
    # iou_threshold is unused by the Gaussian form on either side
    if _hip(boxes):
        from . import hip
        return hip.soft_nms(boxes, scores, iou_threshold, sigma, score_th)
    return eager.soft_nms(boxes, scores, iou_threshold, sigma, score_th)


def soft_nms_batched(boxes, scores, sigma, score_th, conf_th):
    if _hip(boxes):
        from . import hip
        return hip.soft_nms_batched(boxes, scores, sigma, score_th, conf_th)
    return eager.soft_nms_batched(boxes, scores, sigma, score_th, conf_th)


def nms_pack(boxes, classes, scores, box_scale=None, mode=0, iou=0.5,
             sigma=0.5, score_th=0.001, conf=0.0):
    # either NMS mode (0 greedy, 1 Gaussian soft) with a fixed-shape packed
    # result (B, 1+N, 6): one launch and no host sync on GPU (capturable)
    if _hip(boxes):
        from . import hip
        return hip.nms_pack(boxes, classes, scores, box_scale, mode, iou,
                            sigma, score_th, conf)
    return eager.nms_pack(boxes, classes, scores, box_scale, mode, iou,
                          sigma, score_th, conf)


unpack_detections = eager.unpack_detections


def resize_images(img_u8, sizes, T, pretrained=None, dtype=torch.float32):
    # --device-preprocess: Pillow-exact resize (+ normalise) of raw frames
    from . import functional
    return functional.resize_images(img_u8, sizes, T, pretrained, dtype)


def available():
    return _backend.ext() is not None
