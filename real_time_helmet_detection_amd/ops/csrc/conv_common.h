// Shared pieces of the MFMA implicit-GEMM conv family (conv.hip,
// conv_k64.hip, conv_small.hip, conv_halo.hip, conv_fp8.hip,
// conv_halo_fp8.hip): geometry, LDS swizzles, the
// fused epilogue, the 128-B-row double-buffered main loop, the host operand
// preparation and the cross-file host prototypes. Each kernel file keeps
// its tile shape, its fragment reads and its MFMA calls.
#pragma once

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <algorithm>

#include "common.h"

namespace rthd {

using bf16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using i32x8 = __attribute__((ext_vector_type(8))) int;

// global_load_lds operand address spaces
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void glb_void;

struct ConvGeo {
  int B, H, W, Cin, Ho, Wo, Cout;
  int KH, KW, stride, pad;
  int Cinp;   // Cin padded like the packed weights (64; fp8: 128)
  int Coutp;  // Cout padded to 128 (packed-weight rows)
  int M;      // B*Ho*Wo
};

// ------------------------------ device side ---------------------------------

// LDS tile of 64-B rows (32 bf16), 16-B slot swizzle:
//   byte(row, k8) = row*64 + ((k8 ^ ((row>>2)&3))*16)
DEV_INLINE int lds_off_row64(int row, int k8) {
  return row * 64 + ((k8 ^ ((row >> 2) & 3)) << 4);
}
// LDS tile of 128-B rows (64 bf16 / 128 fp8), 16-B chunk swizzle
DEV_INLINE int lds_off_row128(int row, int chunk) {
  return row * 128 + ((chunk ^ (row & 7)) << 4);
}

// output pixel m -> (batch, oy, ox); rows past M decompose pixel 0 (their
// loads are predicated off by the caller's m < M test)
DEV_INLINE void pixel_decompose(int m, const ConvGeo& g, int* b, int* y,
                                int* x) {
  const int mm = m < g.M ? m : 0;
  *b = mm / (g.Ho * g.Wo);
  const int r = mm % (g.Ho * g.Wo);
  *y = r / g.Wo;
  *x = r % g.Wo;
}

// Fused epilogue of one wave's MI x NI 16x16 fragments whose first row is
// row0 and whose first column (for this lane) is col0:
//   y = act(acc*scale[c] + shift[c] (+skip))
// STATS: also emit the wave's column partial sums/sumsq of the stored
// values into sp1/sp2[chunk][Cout] — the training-BN stats then come from
// the fixed-order partial reduce instead of a separate full pass over y
// (cross-lane combine via xor-shuffles: deterministic).
template <int MI, int NI, bool HAS_SKIP, bool STATS, typename OUT_T,
          typename SKIP_T>
DEV_INLINE void conv_epilogue(const f32x4 (&acc)[MI][NI], int row0, int col0,
                              int lane, int M, int Cout,
                              const float* __restrict__ scale,
                              const float* __restrict__ shift,
                              const SKIP_T* __restrict__ skip,
                              OUT_T* __restrict__ y, int act,
                              float* __restrict__ sp1,
                              float* __restrict__ sp2, int64_t chunk) {
  // preload the per-lane scale/shift pairs ONCE (the per-store scalar
  // loads serialized the epilogue: 65 dependent vmcnt(0) waits in the .s)
  float esc[NI], esh[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int c = col0 + ni * 16;
    esc[ni] = c < Cout ? scale[c] : 0.f;
    esh[ni] = c < Cout ? shift[c] : 0.f;
  }
  const int row_in_frag = (lane >> 4) * 4;
  float s1[NI] = {}, s2[NI] = {};
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = row0 + mi * 16 + row_in_frag + r;
      if (m >= M) continue;
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const int c = col0 + ni * 16;
        if (c >= Cout) continue;
        float v = acc[mi][ni][r];
        v = v * esc[ni] + esh[ni];
        if (HAS_SKIP) v += ldf(&skip[(int64_t)m * Cout + c]);
        v = apply_act(v, act);
        stf(&y[(int64_t)m * Cout + c], v);
        if (STATS) {
          s1[ni] += v;
          s2[ni] += v * v;
        }
      }
    }
  }
  if (STATS) {
    // lanes {l, l^16, l^32, l^48} hold the same columns over disjoint
    // rows: fixed-order xor-shuffle combine, lanes 0..15 write the
    // wave's partial row
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      float a = s1[ni], b = s2[ni];
      a += __shfl_xor(a, 16, 64);
      a += __shfl_xor(a, 32, 64);
      b += __shfl_xor(b, 16, 64);
      b += __shfl_xor(b, 32, 64);
      const int c = col0 + ni * 16;
      if ((lane >> 4) == 0 && c < Cout) {
        sp1[chunk * Cout + c] = a;
        sp2[chunk * Cout + c] = b;
      }
    }
  }
}

// Main loop of the 128x128 kernels whose K-step is ONE tap x one 128-B row
// of channels (64 bf16 / 128 fp8): A tile 128 px x 128 B = 16 KB, B tile
// 16 KB, double-buffered in 64 KB of LDS. Staging is async
// global_load_lds: glds j of wave w covers rows (j*4 + w)*8 + lane/8,
// chunk lane&7 (lane-linear 1024-B wave writes); the SOURCE channel chunk
// is pre-swizzled so the image equals lds_off_row128's layout. Each step
// issues the next step's 4+4 glds per thread into the other buffer, calls
// mma(A, B) on this step's tiles, then waits vmcnt(0) and takes a raw
// barrier. Out-of-range pixels source a 16-B zero page.
template <typename T, typename MMA>
DEV_INLINE void conv_mainloop_row128(const T* __restrict__ x,
                                     const T* __restrict__ wpk,
                                     const T* __restrict__ zpage,
                                     const ConvGeo& g, char* lds, int mblk,
                                     int nblk, int wid, int lane, MMA&& mma) {
  constexpr int EPC = 16 / (int)sizeof(T);  // elements per 16-B chunk
  constexpr int KSTEP = 8 * EPC;            // channels per K-step
  const int st_chunk = lane & 7;

  // per-j pixel decomposition for the A rows this thread stages
  int am[4], ab[4], ay[4], ax[4], asw[4];
  const T* aptr[4];
  const T* bptr[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = (j * 4 + wid) * 8 + (lane >> 3);
    am[j] = mblk * 128 + row;
    asw[j] = (st_chunk ^ (row & 7)) * EPC;  // source channel offset
    pixel_decompose(am[j], g, &ab[j], &ay[j], &ax[j]);
    bptr[j] = wpk + ((int64_t)nblk * 128 + row) * g.Cinp + asw[j];
  }

  const int kc = g.Cinp / KSTEP;
  const int taps = g.KH * g.KW;
  const int nsteps = taps * kc;
  const int64_t btap = (int64_t)g.Coutp * g.Cinp;

  int is_step = 0;
  int is_t = 0, is_kb = 0;
  bool avalid[4];
  auto tap_setup = [&]() {
    const int dy_ = is_t / g.KW - g.pad;
    const int dx_ = is_t % g.KW - g.pad;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int iy = ay[j] * g.stride + dy_;
      const int ix = ax[j] * g.stride + dx_;
      avalid[j] = am[j] < g.M && iy >= 0 && iy < g.H && ix >= 0 &&
                  ix < g.W;
      aptr[j] = avalid[j]
          ? x + (((int64_t)ab[j] * g.H + iy) * g.W + ix) * g.Cin + asw[j]
          : zpage;
    }
  };
  tap_setup();

  auto issue_step = [&]() {
    char* base = lds + (is_step & 1) * 32768;
    const int cb = is_kb * KSTEP;
    const int64_t boff = (int64_t)is_t * btap + cb;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const T* a0 = (avalid[j] && cb + asw[j] < g.Cin) ? aptr[j] + cb : zpage;
      __builtin_amdgcn_global_load_lds((glb_void*)a0,
          (lds_void*)(base + (j * 4 + wid) * 1024 + (lane & 63) * 16),
          16, 0, 0);
      __builtin_amdgcn_global_load_lds((glb_void*)(bptr[j] + boff),
          (lds_void*)(base + 16384 + (j * 4 + wid) * 1024 +
                      (lane & 63) * 16), 16, 0, 0);
    }
    ++is_step;
    if (++is_kb == kc) {
      is_kb = 0;
      if (++is_t < taps) tap_setup();
    }
  };

  issue_step();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  for (int step = 0; step < nsteps; ++step) {
    char* A = lds + (step & 1) * 32768;
    char* B = A + 16384;
    if (step + 1 < nsteps) issue_step();

    mma(A, B);

    if (step + 1 < nsteps)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
}

// ------------------------------- host side ----------------------------------

// geometry of a conv over NCHW-logical x, plus the packed-weight shape
// check; cin_pad is the packer's K padding (64 bf16/f32, 128 fp8)
inline ConvGeo make_conv_geo(const char* op, const torch::Tensor& x,
                             const torch::Tensor& wpk, int64_t KH,
                             int64_t KW, int64_t stride, int64_t pad,
                             int64_t Cout, int cin_pad) {
  ConvGeo g;
  g.B = x.size(0);
  g.Cin = x.size(1);
  g.H = x.size(2);
  g.W = x.size(3);
  g.KH = KH; g.KW = KW; g.stride = stride; g.pad = pad;
  g.Ho = (g.H + 2 * g.pad - (int)KH) / (int)stride + 1;
  g.Wo = (g.W + 2 * g.pad - (int)KW) / (int)stride + 1;
  g.Cout = Cout;
  g.Cinp = (int)cdiv(g.Cin, cin_pad) * cin_pad;
  g.Coutp = (int)cdiv(Cout, 128) * 128;
  g.M = g.B * g.Ho * g.Wo;
  TORCH_CHECK(g.Cin >= 1, op, ": bad Cin");
  // 16-B glds chunks must not straddle a pixel (the f32 kernel stages
  // through registers and takes any Cin)
  TORCH_CHECK(wpk.scalar_type() == at::kFloat ||
              g.Cin % (cin_pad / 8) == 0,
              op, ": Cin % ", cin_pad / 8, " required, Cin=", g.Cin);
  TORCH_CHECK(wpk.size(0) == KH * KW && wpk.size(1) == g.Coutp &&
              wpk.size(2) == g.Cinp, op, ": packed weight shape");
  return g;
}

// device operands of one conv call; skip is undefined when there is none
struct ConvOperands {
  torch::Tensor x, wpk, scale, shift, skip, y;
};

// channels-last x and skip cast to io_dtype, float-contiguous scale/shift,
// and a fresh channels-last y of out_dtype
inline ConvOperands prep_conv_operands(
    const ConvGeo& g, const torch::Tensor& x, const torch::Tensor& wpk,
    const torch::Tensor& scale, const torch::Tensor& shift,
    const c10::optional<torch::Tensor>& skip, at::ScalarType io_dtype,
    at::ScalarType out_dtype) {
  ConvOperands o;
  o.wpk = wpk;
  o.x = x.contiguous(at::MemoryFormat::ChannelsLast);
  if (o.x.scalar_type() != io_dtype) o.x = o.x.to(io_dtype);
  o.scale = scale.to(at::kFloat).contiguous();
  o.shift = shift.to(at::kFloat).contiguous();
  if (skip.has_value())
    o.skip = skip->to(io_dtype).contiguous(at::MemoryFormat::ChannelsLast);
  o.y = torch::empty({g.B, (int64_t)g.Cout, g.Ho, g.Wo},
                     o.x.options().dtype(out_dtype)
                         .memory_format(at::MemoryFormat::ChannelsLast));
  return o;
}

template <typename T>
inline T* conv_ptr(const torch::Tensor& t) {
  return t.defined() ? reinterpret_cast<T*>(t.data_ptr()) : nullptr;
}

// per-device cached 16-B zero page (conv.hip)
const bf16* zero_page_bf16(const torch::Tensor& like);

// ---- first-sight measurement of kernel variants (conv.hip, conv_fp8.hip)
// no timing API is legal inside a stream capture: a capturing stream takes
// the caller's heuristic instead
inline bool stream_capturing(hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &st) != hipSuccess) {
    (void)hipGetLastError();
    return true;  // be conservative: never time inside a capture
  }
  return st != hipStreamCaptureStatusNone;
}

// min-of-3 time of fn() in usec on stream s after one warm run (fn must
// enqueue its work on s); synchronizes the stream
template <typename F>
float time_usec(F&& fn, hipStream_t s) {
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  fn();  // warm (code paths, allocator)
  float best = 1e30f;
  for (int r = 0; r < 3; ++r) {
    (void)hipEventRecord(e0, s);
    fn();
    (void)hipEventRecord(e1, s);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    best = std::min(best, ms * 1000.f);
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return best;
}

// variant launchers on prepared bf16 operands: write o.y on the current
// stream. p1/p2 (both or neither; no skip) select the fused-stats epilogue.
void launch_k64(const ConvGeo& g, const ConvOperands& o, int act,
                float* p1, float* p2);                      // conv_k64.hip
void launch_small(const ConvGeo& g, const ConvOperands& o, int act,
                  int splitk);                              // conv_small.hip
// halo-tile 3x3 variant: the shapes it takes, and its launcher
bool halo_eligible(const ConvGeo& g);                       // conv_halo.hip
void launch_halo(const ConvGeo& g, const ConvOperands& o, int act);
// ... with the BN-stats epilogue (halo_stats_ok shapes, no skip): row t of
// p1/p2[halo_stats_rows][ld] = sum / sumsq of tile t's rounded outputs
bool halo_stats_ok(const ConvGeo& g);
int64_t halo_stats_rows(const ConvGeo& g);
void launch_halo_stats(const ConvGeo& g, const ConvOperands& o, int act,
                       float* p1, float* p2, int ld);
// halo-tile fp8 3x3 variant on prepared e4m3 operands  (conv_halo_fp8.hip)
bool fp8_halo_eligible(const ConvGeo& g);
void launch_halo_fp8(const ConvGeo& g, const ConvOperands& o, int act,
                     bool out_fp8);

// python-visible entry points
torch::Tensor pack_weights(torch::Tensor w, bool swap, bool to_bf16);
std::vector<torch::Tensor> pack_weights_pair(torch::Tensor w,
                                             bool to_bf16_fwd,
                                             bool to_bf16_dgrad);
torch::Tensor pack_weights_fp8(torch::Tensor w);
torch::Tensor conv_fwd(torch::Tensor x, torch::Tensor wpk,
                       torch::Tensor scale, torch::Tensor shift,
                       c10::optional<torch::Tensor> skip,
                       int64_t KH, int64_t KW, int64_t stride, int64_t pad,
                       int64_t Cout, int64_t act);
std::vector<torch::Tensor> conv_fwd_stats(
    torch::Tensor x, torch::Tensor wpk, torch::Tensor scale,
    torch::Tensor shift, int64_t KH, int64_t KW, int64_t stride,
    int64_t pad, int64_t Cout, int64_t act, int64_t halo_min_tiles);
std::vector<torch::Tensor> conv_fwd_halo_stats(
    torch::Tensor x, torch::Tensor wpk, torch::Tensor scale,
    torch::Tensor shift, int64_t KH, int64_t KW, int64_t stride, int64_t pad,
    int64_t Cout, int64_t act, c10::optional<torch::Tensor> p1,
    c10::optional<torch::Tensor> p2);
torch::Tensor conv_fwd_k64(torch::Tensor x, torch::Tensor wpk,
                           torch::Tensor scale, torch::Tensor shift,
                           c10::optional<torch::Tensor> skip,
                           int64_t KH, int64_t KW, int64_t stride,
                           int64_t pad, int64_t Cout, int64_t act);
torch::Tensor conv_fwd_halo(torch::Tensor x, torch::Tensor wpk,
                            torch::Tensor scale, torch::Tensor shift,
                            c10::optional<torch::Tensor> skip,
                            int64_t KH, int64_t KW, int64_t stride,
                            int64_t pad, int64_t Cout, int64_t act);
torch::Tensor conv_fwd_small(torch::Tensor x, torch::Tensor wpk,
                             torch::Tensor scale, torch::Tensor shift,
                             c10::optional<torch::Tensor> skip,
                             int64_t KH, int64_t KW, int64_t stride,
                             int64_t pad, int64_t Cout, int64_t act,
                             int64_t splitk);
torch::Tensor conv_fwd_fp8r(torch::Tensor x, torch::Tensor wpk,
                            torch::Tensor scale, torch::Tensor shift,
                            c10::optional<torch::Tensor> skip,
                            int64_t KH, int64_t KW, int64_t stride,
                            int64_t pad, int64_t Cout, int64_t act,
                            bool out_fp8);
// the two kernels conv_fwd_fp8r chooses between, explicitly
torch::Tensor conv_fwd_fp8r_tile128(torch::Tensor x, torch::Tensor wpk,
                                    torch::Tensor scale, torch::Tensor shift,
                                    c10::optional<torch::Tensor> skip,
                                    int64_t KH, int64_t KW, int64_t stride,
                                    int64_t pad, int64_t Cout, int64_t act,
                                    bool out_fp8);
torch::Tensor conv_fwd_fp8r_halo(torch::Tensor x, torch::Tensor wpk,
                                 torch::Tensor scale, torch::Tensor shift,
                                 c10::optional<torch::Tensor> skip,
                                 int64_t KH, int64_t KW, int64_t stride,
                                 int64_t pad, int64_t Cout, int64_t act,
                                 bool out_fp8);
// halo-tile fp8 launches of this process so far (host-side counter)
int64_t fp8_halo_launch_count();

}  // namespace rthd
