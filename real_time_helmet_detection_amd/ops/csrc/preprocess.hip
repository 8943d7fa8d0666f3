// Device-side serving preprocess: the 8-bit antialiased bilinear resample of
// PIL.Image.resize((T, T), BILINEAR) for a batch of raw uint8 frames of
// different sizes, bit for bit, optionally fused with the uint8 -> normalised
// lookup of normalize_u8 (encode.hip). The torch oracle is
// ops.eager.resize_images.
//
// The resample is separable and all-integer once its coefficients exist.
// Per axis (input size n, output size T), in IEEE double, every operation
// rounded on its own (no fma contraction, no fast-math):
//
//   scale = n / T;  fs = max(scale, 1);  support = fs
//   center = (i + 0.5) * scale
//   xmin = max((int)(center - support + 0.5), 0)
//   xmax = min((int)(center + support + 0.5), n) - xmin
//   w[x] = tri((x + xmin - center + 0.5) / fs),  tri(t) = max(1 - |t|, 0)
//   ww = w[0] + ... + w[xmax-1] in that order;  w[x] /= ww when ww != 0
//   k[x] = (int)(0.5 + w[x] * 2^22)
//
// and a pass over that axis is, per channel,
//
//   out = clamp((2^21 + sum_x pixel[xmin + x] * k[x]) >> 22, 0, 255)
//
// horizontal first (rounded to uint8), then vertical over the uint8
// intermediate. A pass over an axis that keeps its size has the single
// coefficient 2^22 and returns its input, so both passes always run.
//
// Two launches per batch, neither reading anything back to the host:
//
// 1. resize_coef_kernel: one lane per (image, axis, output index) builds
//    [xmin, xmax, k[0..kmax-1]] in fp64 from sizes[b], into a workspace
//    whose shape (B, 2, T, kmax + 2) follows from the canvas shape alone:
//    kmax = ceil(max(Hmax, Wmax, T) / T) * 2 + 1 bounds the taps of every
//    image that fits the canvas. The image sizes live on the device (or, for
//    resize_frame, in the launch arguments), which is why the coefficients
//    cannot be built on the host without a synchronising read-back.
// 2. resize_u8_kernel: grid = (tiles of the T x T output, B). A block owns
//    RS_TR rows x RS_TC columns of one image. It stages its rows' and
//    columns' coefficients in LDS, runs the horizontal pass for the band of
//    source rows its output rows touch (first row's xmin to last row's
//    xmin + xmax) into an LDS uint8 intermediate, then the vertical pass
//    from LDS, then the table lookup and the stores: PX consecutive pixels
//    per lane as vector stores when the group is full and aligned, element
//    by element otherwise (as augment.hip).
//
// Addressing cannot leave an allocation whatever sizes holds: h and w are
// clamped into the canvas, tap counts into kmax, band rows into the LDS
// band, and every tap index into its own image. No atomics, no memset,
// every output and workspace element written: bitwise deterministic and
// legal under stream capture.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include "common.h"

namespace rthd {

constexpr int RS_THREADS = 256;
constexpr int RS_TR = 8;    // output rows per block
constexpr int RS_TC = 32;   // output columns per block
static_assert(RS_TR * RS_TC == RS_THREADS, "one lane per tile pixel");
// largest per-axis minification ceil(n / T) the LDS layout is sized for
constexpr int RS_MAX_RATIO = 16;
constexpr int RS_KCAP = RS_MAX_RATIO * 2 + 1;  // taps at that ratio
// source rows under RS_TR output rows: the xmin of the last row is at most
// floor((RS_TR - 1) * scale) + 1 past the first row's, plus its own taps
constexpr int RS_BAND_CAP = (RS_TR - 1) * RS_MAX_RATIO + 1 + RS_KCAP;
constexpr int RS_PREC = 22;  // coefficient precision bits

template <typename Out> struct ResizeIO;
template <> struct ResizeIO<uint8_t> {  // 4 pixels = 12 B (3 x 4 B)
  using vec = uint32_t;
  static constexpr int PX = 4;
};
template <> struct ResizeIO<float> {    // 4 pixels = 48 B (3 x 16 B)
  using vec = uint4;
  static constexpr int PX = 4;
};
template <> struct ResizeIO<uint16_t> {  // bf16: 8 pixels = 48 B (3 x 16 B)
  using vec = uint4;
  static constexpr int PX = 8;
};

// image b's [h, w]: from the device table, or (resize_frame) the launch
// arguments; clamped into the canvas either way
DEV_INLINE void rs_size(const int* __restrict__ sizes, int b, int h_arg,
                        int w_arg, int Hmax, int Wmax, int& h, int& w) {
  h = sizes ? sizes[b * 2 + 0] : h_arg;
  w = sizes ? sizes[b * 2 + 1] : w_arg;
  h = min(max(h, 1), Hmax);
  w = min(max(w, 1), Wmax);
}

DEV_INLINE double rs_tri(double t) {
#pragma clang fp contract(off)
  t = fabs(t);
  return t < 1.0 ? 1.0 - t : 0.0;
}

// coef (B, 2, T, kmax + 2) int32: axis 0 = x (from w), axis 1 = y (from h);
// per output index [xmin, xmax, k[0..kmax-1]], k zero past xmax.
__global__ void __launch_bounds__(RS_THREADS)
resize_coef_kernel(const int* __restrict__ sizes, int h_arg, int w_arg,
                   int* __restrict__ coef, float* __restrict__ scale_out,
                   int B, int Hmax, int Wmax, int T, int kmax) {
#pragma clang fp contract(off)
  const int64_t idx = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
  if (scale_out != nullptr && idx == 0) {
    // resize_frame: network pixels -> frame pixels, per box coordinate
    const float sx = (float)((double)w_arg / (double)T);
    const float sy = (float)((double)h_arg / (double)T);
    scale_out[0] = sx;
    scale_out[1] = sy;
    scale_out[2] = sx;
    scale_out[3] = sy;
  }
  if (idx >= (int64_t)B * 2 * T) return;
  const int i = (int)(idx % T);
  const int axis = (int)((idx / T) & 1);
  const int b = (int)(idx / (2 * (int64_t)T));
  int h, w;
  rs_size(sizes, b, h_arg, w_arg, Hmax, Wmax, h, w);
  const int n = axis == 0 ? w : h;

  const double scale = (double)n / (double)T;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = fs;
  const double center = ((double)i + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  xmin = min(max(xmin, 0), n - 1);
  int xmax = (int)(center + support + 0.5);
  xmax = min(xmax, n);
  const int cnt = min(max(xmax - xmin, 0), kmax);

  double ww = 0.0;
  for (int x = 0; x < cnt; ++x)
    ww += rs_tri(((double)(x + xmin) - center + 0.5) / fs);

  int* __restrict__ o = coef + idx * (kmax + 2);
  o[0] = xmin;
  o[1] = cnt;
  for (int x = 0; x < kmax; ++x) {
    int k = 0;
    if (x < cnt) {
      double wx = rs_tri(((double)(x + xmin) - center + 0.5) / fs);
      if (ww != 0.0) wx /= ww;
      k = (int)(0.5 + wx * (double)(1 << RS_PREC));
    }
    o[2 + x] = k;
  }
}

// one tile axis of the coefficient table -> LDS
DEV_INLINE void rs_stage(const int* __restrict__ src, int count, int ks,
                         int* mins, int* cnts, int* k) {
  for (int t = threadIdx.x; t < count * ks; t += RS_THREADS) {
    const int c = t / ks, j = t - c * ks;
    const int v = src[t];
    if (j == 0) mins[c] = v;
    else if (j == 1) cnts[c] = min(max(v, 0), ks - 2);
    else k[c * RS_KCAP + (j - 2)] = v;
  }
}

DEV_INLINE uint8_t rs_round(uint32_t acc) {
  return (uint8_t)min(acc >> RS_PREC, 255u);
}

template <typename Out>
__global__ void __launch_bounds__(RS_THREADS)
resize_u8_kernel(const uint8_t* __restrict__ in,   // (B,Hmax,Wmax,3)
                 const int* __restrict__ sizes,    // (B,2) [h, w] | null
                 int h_arg, int w_arg,
                 const int* __restrict__ coef,     // (B,2,T,kmax+2)
                 const Out* __restrict__ table,    // [3][256] | unused
                 Out* __restrict__ out,            // (B,T,T,3)
                 int Hmax, int Wmax, int T, int kmax) {
  using IO = ResizeIO<Out>;
  using vec = typename IO::vec;
  constexpr int PX = IO::PX;
  constexpr int NEL = 3 * PX;
  constexpr int PERV = (int)(sizeof(vec) / sizeof(Out));
  constexpr int GPR = RS_TC / PX;  // lane groups per tile row
  constexpr bool LUT = sizeof(Out) != 1;

  __shared__ Out tab[LUT ? 3 * 256 : 1];
  __shared__ int kx[RS_TC * RS_KCAP], ky[RS_TR * RS_KCAP];
  __shared__ int xmin_s[RS_TC], xcnt_s[RS_TC], ymin_s[RS_TR], ycnt_s[RS_TR];
  __shared__ uint8_t band[RS_BAND_CAP * RS_TC * 3];
  __shared__ uint8_t qt[RS_TR * RS_TC * 3];

  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const int tiles_x = (T + RS_TC - 1) / RS_TC;
  const int row0 = (int)(blockIdx.x / tiles_x) * RS_TR;
  const int col0 = (int)(blockIdx.x % tiles_x) * RS_TC;
  const int nrows = min(RS_TR, T - row0);
  const int ncols = min(RS_TC, T - col0);
  int h, w;
  rs_size(sizes, b, h_arg, w_arg, Hmax, Wmax, h, w);

  const int ks = kmax + 2;
  const int* __restrict__ cb = coef + (int64_t)b * 2 * T * ks;
  rs_stage(cb + (int64_t)col0 * ks, ncols, ks, xmin_s, xcnt_s, kx);
  rs_stage(cb + ((int64_t)T + row0) * ks, nrows, ks, ymin_s, ycnt_s, ky);
  if constexpr (LUT) {
    for (int i = tid; i < 3 * 256; i += RS_THREADS) tab[i] = table[i];
  }
  __syncthreads();

  // horizontal pass over the band of source rows under this tile's rows
  const int y0 = ymin_s[0];
  const int nb = min(max(ymin_s[nrows - 1] + ycnt_s[nrows - 1] - y0, 0),
                     RS_BAND_CAP);
  const uint8_t* __restrict__ img = in + (int64_t)b * Hmax * Wmax * 3;
  for (int t = tid; t < nb * ncols; t += RS_THREADS) {
    const int r = t / ncols, c = t - r * ncols;
    const int yy = min(max(y0 + r, 0), h - 1);
    const uint8_t* __restrict__ row = img + yy * (Wmax * 3);
    const int xm = xmin_s[c], cnt = xcnt_s[c];
    const int* __restrict__ k = kx + c * RS_KCAP;
    uint32_t a0 = 1u << (RS_PREC - 1), a1 = a0, a2 = a0;
    for (int x = 0; x < cnt; ++x) {
      const int xx = min(max(xm + x, 0), w - 1);
      const uint8_t* __restrict__ p = row + xx * 3;
      const uint32_t kk = (uint32_t)k[x];
      a0 += __umul24(p[0], kk);
      a1 += __umul24(p[1], kk);
      a2 += __umul24(p[2], kk);
    }
    uint8_t* __restrict__ d = band + (r * RS_TC + c) * 3;
    d[0] = rs_round(a0);
    d[1] = rs_round(a1);
    d[2] = rs_round(a2);
  }
  __syncthreads();

  // vertical pass from the band: one lane per tile pixel
  {
    const int r = tid / RS_TC, c = tid - r * RS_TC;
    if (r < nrows && c < ncols) {
      const int off = ymin_s[r] - y0, cnt = ycnt_s[r];
      const int* __restrict__ k = ky + r * RS_KCAP;
      uint32_t a0 = 1u << (RS_PREC - 1), a1 = a0, a2 = a0;
      for (int x = 0; x < cnt; ++x) {
        const int rr = min(max(off + x, 0), RS_BAND_CAP - 1);
        const uint8_t* __restrict__ p = band + (rr * RS_TC + c) * 3;
        const uint32_t kk = (uint32_t)k[x];
        a0 += __umul24(p[0], kk);
        a1 += __umul24(p[1], kk);
        a2 += __umul24(p[2], kk);
      }
      uint8_t* __restrict__ d = qt + (r * RS_TC + c) * 3;
      d[0] = rs_round(a0);
      d[1] = rs_round(a1);
      d[2] = rs_round(a2);
    }
  }
  __syncthreads();

  // lookup + stores: a lane owns PX consecutive pixels of one row
  if (tid >= RS_TR * GPR) return;
  const int r = tid / GPR;
  const int xl = (tid - r * GPR) * PX;
  if (r >= nrows || xl >= ncols) return;
  const int nvalid = min(PX, ncols - xl);
  alignas(16) Out v[NEL];
  const uint8_t* __restrict__ q = qt + (r * RS_TC + xl) * 3;
#pragma unroll
  for (int k = 0; k < NEL; ++k) {
    // pixels past nvalid were never computed: whatever byte is there maps
    // to some table entry and is not stored
    if constexpr (LUT) {
      v[k] = tab[(k % 3) * 256 + q[k]];
    } else {
      v[k] = (Out)q[k];
    }
  }
  Out* __restrict__ o =
      out + (((int64_t)b * T + row0 + r) * T + col0 + xl) * 3;
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
static void resize_launch(const torch::Tensor& in, const int* sizes, int h,
                          int w, const int* coef, const Out* table, Out* out,
                          int64_t T, int kmax) {
  const int64_t tiles = cdiv(T, RS_TC) * cdiv(T, RS_TR);
  dim3 grid((unsigned)tiles, (unsigned)in.size(0));
  auto s = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(resize_u8_kernel<Out>, grid, dim3(RS_THREADS), 0, s,
      in.data_ptr<uint8_t>(), sizes, h, w, coef, table, out,
      (int)in.size(1), (int)in.size(2), (int)T, kmax);
  HIP_CHECK_LAST();
}

// in_: contiguous (B,Hmax,Wmax,3) uint8. sizes null: every image is h x w
// (the launch arguments). scale_out: 4 floats or null.
static torch::Tensor resize_impl(const char* name, const torch::Tensor& in_,
                                 const int* sizes, int h, int w, int64_t T,
                                 const c10::optional<torch::Tensor>& table,
                                 float* scale_out) {
  const int64_t B = in_.size(0), Hmax = in_.size(1), Wmax = in_.size(2);
  TORCH_CHECK(T >= 1, name, ": T must be >= 1");
  TORCH_CHECK(B == 0 || (Hmax >= 1 && Wmax >= 1), name, ": empty canvas");
  // in-image byte offsets and the tile index are 32-bit
  TORCH_CHECK(Hmax * Wmax * 3 < (1LL << 31) && T < (1LL << 20) &&
                  B <= 65535,
              name, ": shape out of range");
  const int64_t ratio = cdiv(std::max(std::max(Hmax, Wmax), T), T);
  TORCH_CHECK(B == 0 || ratio <= RS_MAX_RATIO, name, ": the canvas (", Hmax,
              " x ", Wmax, ") is more than ", RS_MAX_RATIO,
              " times the output side ", T, " on one axis; per-axis "
              "minification is supported up to ", RS_MAX_RATIO, "x");
  const int kmax = (int)ratio * 2 + 1;
  bool is_bf16 = false;
  if (table.has_value()) {
    is_bf16 = table->scalar_type() == at::kBFloat16;
    TORCH_CHECK(table->is_cuda() && table->device() == in_.device() &&
                    table->numel() == 3 * 256 &&
                    (is_bf16 || table->scalar_type() == at::kFloat),
                name, ": table must be (3,256) float32 or bfloat16");
  }
  auto out = torch::empty(
      {B, T, T, 3}, table.has_value() ? table->options() : in_.options());
  if (B > 0) {
    auto coef = torch::empty({B, 2, T, kmax + 2},
                             in_.options().dtype(at::kInt));
    auto s = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(resize_coef_kernel,
        dim3((unsigned)cdiv(B * 2 * T, RS_THREADS)), dim3(RS_THREADS), 0, s,
        sizes, h, w, coef.data_ptr<int>(), scale_out, (int)B, (int)Hmax,
        (int)Wmax, (int)T, kmax);
    HIP_CHECK_LAST();
    const int* cf = coef.data_ptr<int>();
    if (!table.has_value()) {
      resize_launch<uint8_t>(in_, sizes, h, w, cf, nullptr,
                             out.data_ptr<uint8_t>(), T, kmax);
    } else {
      auto table_ = table->contiguous();
      if (is_bf16) {
        resize_launch<uint16_t>(
            in_, sizes, h, w, cf,
            reinterpret_cast<const uint16_t*>(table_.data_ptr()),
            reinterpret_cast<uint16_t*>(out.data_ptr()), T, kmax);
      } else {
        resize_launch<float>(in_, sizes, h, w, cf, table_.data_ptr<float>(),
                             out.data_ptr<float>(), T, kmax);
      }
    }
  }
  return table.has_value() ? out.permute({0, 3, 1, 2}) : out;
}

// table absent: (B,T,T,3) uint8. table (3,256) fp32 | bf16: the normalised
// image as a (B,3,T,T) channels_last view of the NHWC storage.
torch::Tensor resize_u8(torch::Tensor img_u8, torch::Tensor sizes, int64_t T,
                        c10::optional<torch::Tensor> table) {
  TORCH_CHECK(img_u8.is_cuda() && img_u8.scalar_type() == at::kByte &&
                  img_u8.dim() == 4 && img_u8.size(3) == 3,
              "resize_u8: image must be a (B,Hmax,Wmax,3) uint8 device "
              "tensor");
  TORCH_CHECK(sizes.is_cuda() && sizes.scalar_type() == at::kInt &&
                  sizes.dim() == 2 && sizes.size(0) == img_u8.size(0) &&
                  sizes.size(1) == 2,
              "resize_u8: sizes must be a (B,2) int32 device tensor");
  TORCH_CHECK(sizes.device() == img_u8.device(),
              "resize_u8: tensors must share one device");
  auto in_ = img_u8.contiguous();
  auto sizes_ = sizes.contiguous();
  return resize_impl("resize_u8", in_, sizes_.data_ptr<int>(), 0, 0, T,
                     table, nullptr);
}

// One raw frame of any size -> (normalised (1,3,T,T) image, (4,) fp32
// [W/T, H/T, W/T, H/T]). H and W are read from the tensor at run time and
// reach the kernels as launch arguments; the scale vector is written by the
// coefficient kernel, so there is no host-to-device copy.
std::tuple<torch::Tensor, torch::Tensor> resize_frame(torch::Tensor frame_u8,
                                                      int64_t T,
                                                      torch::Tensor table) {
  TORCH_CHECK(frame_u8.is_cuda() && frame_u8.scalar_type() == at::kByte &&
                  frame_u8.dim() == 3 && frame_u8.size(2) == 3 &&
                  frame_u8.size(0) >= 1 && frame_u8.size(1) >= 1,
              "resize_frame: frame must be a non-empty (H,W,3) uint8 device "
              "tensor");
  auto in_ = frame_u8.contiguous().unsqueeze(0);
  auto scale = torch::empty({4}, in_.options().dtype(at::kFloat));
  auto image = resize_impl("resize_frame", in_, nullptr, (int)in_.size(1),
                           (int)in_.size(2), T, table,
                           scale.data_ptr<float>());
  return {image, scale};
}

int64_t resize_max_ratio() { return RS_MAX_RATIO; }

}  // namespace rthd
