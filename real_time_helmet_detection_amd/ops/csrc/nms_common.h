// Box helpers shared by the hard (nms.hip) and soft (soft_nms.hip) NMS
// kernels: one IoU form for both, the one ops/eager.py box_iou defines
// (clamped widths and areas, no +1, union clamped at 1e-9).
#pragma once

#include "common.h"

namespace rthd {

// per-image candidate limit of the LDS-resident NMS kernels
constexpr int NMS_CAP = 2048;

DEV_INLINE float box_area(float x1, float y1, float x2, float y2) {
  return fmaxf(x2 - x1, 0.f) * fmaxf(y2 - y1, 0.f);
}

// IoU of xyxy boxes a and b; area_a is passed in because both kernels hold
// box a fixed over an inner loop
DEV_INLINE float box_iou(float ax1, float ay1, float ax2, float ay2,
                         float area_a, float bx1, float by1, float bx2,
                         float by2) {
  const float xx1 = fmaxf(ax1, bx1);
  const float yy1 = fmaxf(ay1, by1);
  const float xx2 = fminf(ax2, bx2);
  const float yy2 = fminf(ay2, by2);
  const float inter = fmaxf(xx2 - xx1, 0.f) * fmaxf(yy2 - yy1, 0.f);
  const float area_b = box_area(bx1, by1, bx2, by2);
  const float uni = area_a + area_b - inter;
  return inter / fmaxf(uni, 1e-9f);
}

}  // namespace rthd
