// Device-side train augmentation: brightness multiply, affine (scale about
// the centre + translate), crop-keep-size, horizontal flip and the batch
// resize of data.augment.TrainAugmentor as ONE gather per batch, optionally
// fused with the uint8 -> normalised lookup of normalize_u8 (encode.hip).
//
// Everything the augmentor does to pixels is elementwise or an axis-aligned
// resample, so the whole chain collapses on the host to one map per image
// and axis, src = a * out + b (continuous coordinates, pixel i centred at
// i + 0.5), plus the brightness factor. Per output pixel, in fp32, in this
// order, without fma contraction (the torch oracle ops.eager.augment_images
// rounds after every operation):
//
//   xs = a*(x + 0.5) + b;  g = xs - 0.5;  x0 = floor(g);  fx = g - x0
//   tap(p) = in the image ? min(floor(p * factor), 255) : 0   (black fill)
//   top = v00*(1-fx) + v01*fx;  bot = v10*(1-fx) + v11*fx
//   v   = top*(1-fy) + bot*fy;  q = clamp((int)floor(v + 0.5), 0, 255)
//
// q is stored as uint8, or looked up in the 3x256 normalise table (LDS), so
// the normalised output is bit-identical to normalize_images(q).
//
// Layout: the batch is one (B, Hmax, Wmax, 3) uint8 canvas; image b lives
// in its top-left sizes[b] = (h, w) corner. grid = (tiles of the T x T
// output, B), so sizes[b] and coef[b] are wave-uniform loads. A lane owns
// PX consecutive output x of one row and writes them as three vector
// stores when the group is full and its address aligned, element by
// element otherwise (row tail, rows off the 16-byte grid).
//
// Addressing is branch-free and cannot leave the allocation whatever the
// coefficients are: h and w are clamped into the canvas, g is clamped to
// [-2, n + 1] before the int cast (which changes no result: every tap of a
// clamped g is outside the image), every tap index is clamped into
// [0, n - 1] of its own image, and the loaded value is multiplied by the
// in-image mask. No atomics, no memset, every output element written:
// bitwise deterministic and legal under stream capture.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include "common.h"

namespace rthd {

constexpr int AUG_THREADS = 256;

template <typename Out> struct AugIO;
// uint8: 4 pixels per lane = 12 B out (3 x 4 B)
template <> struct AugIO<uint8_t> {
  using vec = uint32_t;
  static constexpr int PX = 4;
};
// fp32: 4 pixels per lane = 48 B out (3 x 16 B)
template <> struct AugIO<float> {
  using vec = uint4;
  static constexpr int PX = 4;
};
// bf16: 8 pixels per lane = 48 B out (3 x 16 B)
template <> struct AugIO<uint16_t> {
  using vec = uint4;
  static constexpr int PX = 8;
};

// one axis of the map for output index i: clamped tap indices c0/c1, their
// in-image masks m0/m1 and the fractional weight f
DEV_INLINE void aug_axis(float a, float b, int i, int n, int& c0, int& c1,
                         float& m0, float& m1, float& f) {
#pragma clang fp contract(off)
  const float s = a * ((float)i + 0.5f) + b;
  float g = s - 0.5f;
  g = fminf(fmaxf(g, -2.0f), (float)n + 1.0f);
  const float g0 = floorf(g);
  f = g - g0;
  const int i0 = (int)g0, i1 = i0 + 1;
  m0 = (i0 >= 0 && i0 < n) ? 1.0f : 0.0f;
  m1 = (i1 >= 0 && i1 < n) ? 1.0f : 0.0f;
  c0 = min(max(i0, 0), n - 1);
  c1 = min(max(i1, 0), n - 1);
}

DEV_INLINE float aug_tap(const uint8_t* __restrict__ p, float factor,
                         float mask) {
#pragma clang fp contract(off)
  return fminf(floorf((float)(*p) * factor), 255.0f) * mask;
}

template <typename Out>
__global__ void __launch_bounds__(AUG_THREADS)
augment_u8_kernel(const uint8_t* __restrict__ in,   // (B,Hmax,Wmax,3)
                  const int* __restrict__ sizes,    // (B,2) [h, w]
                  const float* __restrict__ coef,   // (B,5) ax bx ay by f
                  const Out* __restrict__ table,    // [3][256] | unused
                  Out* __restrict__ out,            // (B,T,T,3)
                  int Hmax, int Wmax, int T) {
#pragma clang fp contract(off)
  using IO = AugIO<Out>;
  using vec = typename IO::vec;
  constexpr int PX = IO::PX;
  constexpr int NEL = 3 * PX;
  constexpr int PERV = (int)(sizeof(vec) / sizeof(Out));
  constexpr bool LUT = sizeof(Out) != 1;

  __shared__ Out tab[LUT ? 3 * 256 : 1];
  if constexpr (LUT) {
    for (int i = threadIdx.x; i < 3 * 256; i += AUG_THREADS)
      tab[i] = table[i];
    __syncthreads();
  }

  const int b = blockIdx.y;
  const int h = min(max(sizes[b * 2 + 0], 1), Hmax);
  const int w = min(max(sizes[b * 2 + 1], 1), Wmax);
  const float ax = coef[b * 5 + 0], bx = coef[b * 5 + 1];
  const float ay = coef[b * 5 + 2], by = coef[b * 5 + 3];
  const float factor = coef[b * 5 + 4];

  const int gpr = (T + PX - 1) / PX;  // lane groups per output row
  const int g = blockIdx.x * AUG_THREADS + threadIdx.x;
  if (g >= T * gpr) return;
  const int y = g / gpr;
  const int x0 = (g - y * gpr) * PX;

  int cy0, cy1;
  float my0, my1, fy;
  aug_axis(ay, by, y, h, cy0, cy1, my0, my1, fy);
  const uint8_t* __restrict__ img = in + (int64_t)b * Hmax * Wmax * 3;
  const uint8_t* __restrict__ r0 = img + cy0 * (Wmax * 3);
  const uint8_t* __restrict__ r1 = img + cy1 * (Wmax * 3);
  const float gy = 1.0f - fy;

  alignas(16) Out v[NEL];
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    // a tail lane computes its columns past T too (every address is
    // clamped) and simply does not store them
    int cx0, cx1;
    float mx0, mx1, fx;
    aug_axis(ax, bx, x0 + k, w, cx0, cx1, mx0, mx1, fx);
    const float gx = 1.0f - fx;
    const float m00 = my0 * mx0, m01 = my0 * mx1;
    const float m10 = my1 * mx0, m11 = my1 * mx1;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v00 = aug_tap(r0 + cx0 * 3 + c, factor, m00);
      const float v01 = aug_tap(r0 + cx1 * 3 + c, factor, m01);
      const float v10 = aug_tap(r1 + cx0 * 3 + c, factor, m10);
      const float v11 = aug_tap(r1 + cx1 * 3 + c, factor, m11);
      const float top = v00 * gx + v01 * fx;
      const float bot = v10 * gx + v11 * fx;
      const float val = top * gy + bot * fy;
      const int q = min(max((int)floorf(val + 0.5f), 0), 255);
      if constexpr (LUT) {
        v[k * 3 + c] = tab[c * 256 + q];
      } else {
        v[k * 3 + c] = (Out)q;
      }
    }
  }

  Out* __restrict__ o = out + (((int64_t)b * T + y) * T + x0) * 3;
  const int nvalid = min(PX, T - x0);
  if (nvalid == PX &&
      (reinterpret_cast<uintptr_t>(o) & (sizeof(vec) - 1)) == 0) {
    vec* ov = reinterpret_cast<vec*>(o);
#pragma unroll
    for (int i = 0; i < NEL / PERV; ++i)
      ov[i] = *reinterpret_cast<const vec*>(&v[i * PERV]);
  } else {
#pragma unroll
    for (int k = 0; k < NEL; ++k)
      if (k < nvalid * 3) o[k] = v[k];
  }
}

template <typename Out>
static void aug_launch(const torch::Tensor& in, const torch::Tensor& sizes,
                       const torch::Tensor& coef, const Out* table, Out* out,
                       int64_t T) {
  const int64_t B = in.size(0);
  const int64_t groups = T * cdiv(T, AugIO<Out>::PX);
  dim3 grid((unsigned)cdiv(groups, AUG_THREADS), (unsigned)B);
  auto s = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(augment_u8_kernel<Out>, grid, dim3(AUG_THREADS), 0, s,
      in.data_ptr<uint8_t>(), sizes.data_ptr<int>(), coef.data_ptr<float>(),
      table, out, (int)in.size(1), (int)in.size(2), (int)T);
  HIP_CHECK_LAST();
}

// table absent: (B,T,T,3) uint8. table (3,256) fp32 | bf16: the normalised
// image as a (B,3,T,T) channels_last view of the NHWC storage.
torch::Tensor augment_u8(torch::Tensor img_u8, torch::Tensor sizes,
                         torch::Tensor coef, int64_t T,
                         c10::optional<torch::Tensor> table) {
  TORCH_CHECK(img_u8.is_cuda() && img_u8.scalar_type() == at::kByte &&
                  img_u8.dim() == 4 && img_u8.size(3) == 3,
              "augment_u8: image must be a (B,Hmax,Wmax,3) uint8 device "
              "tensor");
  const int64_t B = img_u8.size(0), Hmax = img_u8.size(1),
                Wmax = img_u8.size(2);
  TORCH_CHECK(sizes.is_cuda() && sizes.scalar_type() == at::kInt &&
                  sizes.dim() == 2 && sizes.size(0) == B &&
                  sizes.size(1) == 2,
              "augment_u8: sizes must be a (B,2) int32 device tensor");
  TORCH_CHECK(coef.is_cuda() && coef.scalar_type() == at::kFloat &&
                  coef.dim() == 2 && coef.size(0) == B && coef.size(1) == 5,
              "augment_u8: coef must be a (B,5) float32 device tensor");
  TORCH_CHECK(sizes.device() == img_u8.device() &&
                  coef.device() == img_u8.device(),
              "augment_u8: tensors must share one device");
  TORCH_CHECK(T >= 1, "augment_u8: T must be >= 1");
  TORCH_CHECK(B == 0 || (Hmax >= 1 && Wmax >= 1),
              "augment_u8: empty canvas");
  // in-image byte offsets and the lane-group index are 32-bit
  TORCH_CHECK(Hmax * Wmax * 3 < (1LL << 31) && T * (T + 8) < (1LL << 31) &&
                  B <= 65535,
              "augment_u8: shape out of range");
  bool is_bf16 = false;
  if (table.has_value()) {
    is_bf16 = table->scalar_type() == at::kBFloat16;
    TORCH_CHECK(table->is_cuda() && table->device() == img_u8.device() &&
                    table->numel() == 3 * 256 &&
                    (is_bf16 || table->scalar_type() == at::kFloat),
                "augment_u8: table must be (3,256) float32 or bfloat16");
  }
  auto in_ = img_u8.contiguous();
  auto sizes_ = sizes.contiguous();
  auto coef_ = coef.contiguous();
  auto out = torch::empty(
      {B, T, T, 3},
      table.has_value() ? table->options() : in_.options());
  if (B > 0) {
    if (!table.has_value()) {
      aug_launch<uint8_t>(in_, sizes_, coef_, nullptr,
                          out.data_ptr<uint8_t>(), T);
    } else {
      auto table_ = table->contiguous();
      if (is_bf16) {
        aug_launch<uint16_t>(
            in_, sizes_, coef_,
            reinterpret_cast<const uint16_t*>(table_.data_ptr()),
            reinterpret_cast<uint16_t*>(out.data_ptr()), T);
      } else {
        aug_launch<float>(in_, sizes_, coef_, table_.data_ptr<float>(),
                          out.data_ptr<float>(), T);
      }
    }
  }
  return table.has_value() ? out.permute({0, 3, 1, 2}) : out;
}

}  // namespace rthd
