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

// ---- packed emit (nms_pack) -------------------------------------------
// Both kernels have a PACK instantiation that writes, per image, a
// (1 + N, 6) fp32 block instead of index lists: row 0 = [count, 0...], rows
// 1..count = [x1, y1, x2, y2, score, class] in selection order, the rest 0.
// The kernel stores every element of the block exactly once.
constexpr int NMS_REC = 6;

struct NmsPack {
  const int64_t* classes;  // (B,N)
  const float* scale;      // (4,) or (B,4) x,y,x,y multipliers, or null
  float* out;              // (B,1+N,6)
  int scale_stride;        // 0 for (4,), 4 for (B,4)
};

// rows are 24 B, so 8 B aligned whatever the row index
DEV_INLINE void nms_pack_store(float* __restrict__ row, float a, float b,
                               float c, float d, float e, float f) {
  float2* r = reinterpret_cast<float2*>(row);
  r[0] = make_float2(a, b);
  r[1] = make_float2(c, d);
  r[2] = make_float2(e, f);
}

// one selected box -> row 1 + k of the image's block. k < N and orig < N
// are checked here, so no score pattern can move a store or the class
// gather out of the image's slice.
DEV_INLINE void nms_pack_record(const NmsPack& pk, int bimg, int N, int k,
                                int orig, float x1, float y1, float x2,
                                float y2, float score) {
  if ((unsigned)k >= (unsigned)N) return;
  float cls = 0.f;
  if ((unsigned)orig < (unsigned)N)
    cls = (float)pk.classes[(int64_t)bimg * N + orig];
  if (pk.scale != nullptr) {
    const float* sc = pk.scale + (int64_t)bimg * pk.scale_stride;
    // plain fp32 products (nothing to contract with)
    x1 = x1 * sc[0];
    y1 = y1 * sc[1];
    x2 = x2 * sc[2];
    y2 = y2 * sc[3];
  }
  float* base = pk.out + (int64_t)bimg * (1 + N) * NMS_REC;
  nms_pack_store(base + (int64_t)(1 + k) * NMS_REC, x1, y1, x2, y2, score,
                 cls);
}

// header row and the zero tail (rows 1 + count .. N), strided over `nthr`
// threads
DEV_INLINE void nms_pack_finish(const NmsPack& pk, int bimg, int N,
                                int count, int tid, int nthr) {
  float* base = pk.out + (int64_t)bimg * (1 + N) * NMS_REC;
  count = min(max(count, 0), N);
  if (tid == 0) nms_pack_store(base, (float)count, 0.f, 0.f, 0.f, 0.f, 0.f);
  for (int r = count + tid; r < N; r += nthr)
    nms_pack_store(base + (int64_t)(1 + r) * NMS_REC, 0.f, 0.f, 0.f, 0.f,
                   0.f, 0.f);
}

}  // namespace rthd
