// bf16 implicit-GEMM conv variant with a 64-channel K-step.
//
// The 32-ch-per-step kernel (conv.hip) measures ~20-26% of the bf16 MFMA
// peak: per-step glds ISSUE cost + the barrier cadence dominate (guide
// §"LDS-DMA piece issue cost": ~60-185 cyc per piece). The fp8 K=128
// kernel demonstrated that amortizing those over more channels per
// barrier is worth +24-52% on the big shapes. This is the bf16 analog:
// one K-step = one tap x 64 channels — A tile 128 px x 64 bf16 = 16 KB,
// B tile 16 KB, double-buffered 64 KB LDS (2 blocks/CU), 8 glds and 32
// MFMA per step (twice the MFMA per barrier of conv.hip), lane-linear
// glds image with the chunk^(row&7) swizzle reversed at the b128
// fragment reads (staging loop: conv_mainloop_row128 in conv_common.h).
// Selected per shape by the conv_fwd autotune cache.
#include "conv_common.h"

namespace rthd {

template <bool HAS_SKIP, bool STATS = false>
__global__ __launch_bounds__(256)
void conv_fwd_bf16_k64_kernel(const bf16* __restrict__ x,
                              const bf16* __restrict__ wpk,
                              const float* __restrict__ scale,
                              const float* __restrict__ shift,
                              const bf16* __restrict__ skip,
                              const bf16* __restrict__ zpage,
                              bf16* __restrict__ y,
                              ConvGeo g, int act,
                              float* __restrict__ sp1 = nullptr,
                              float* __restrict__ sp2 = nullptr) {
  const int mblk = blockIdx.x;
  const int nblk = blockIdx.y;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  // 2 x (A 16KB | B 16KB)

  f32x4 acc[4][4] = {};

  conv_mainloop_row128<bf16>(x, wpk, zpage, g, smem, mblk, nblk, wid, lane,
                             [&](const char* A, const char* B) {
    const int arow_base = wr * 64 + (lane & 15);
    const int brow_base = wc * 64 + (lane & 15);
    const int k8 = lane >> 4;
#pragma unroll
    for (int h = 0; h < 2; ++h) {  // two 32-ch halves of the 64-ch step
      bf16x8 afrag[4], bfrag[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        afrag[i] = *reinterpret_cast<const bf16x8*>(
            A + lds_off_row128(arow_base + 16 * i, h * 4 + k8));
        bfrag[i] = *reinterpret_cast<const bf16x8*>(
            B + lds_off_row128(brow_base + 16 * i, h * 4 + k8));
      }
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afrag[mi], bfrag[ni], acc[mi][ni], 0, 0, 0);
    }
  });

  // stats partial row: chunk = mblk*2 + wr
  conv_epilogue<4, 4, HAS_SKIP, STATS>(
      acc, mblk * 128 + wr * 64, nblk * 128 + wc * 64 + (lane & 15), lane,
      g.M, g.Cout, scale, shift, skip, y, act, sp1, sp2,
      (int64_t)mblk * 2 + wr);
}

// p1/p2 non-null: fused-stats epilogue (no skip — training BN runs the
// conv linear; skip/act fuse later in bn_act_fwd). p1/p2: [2*Mblks, Cout].
void launch_k64(const ConvGeo& g, const ConvOperands& o, int act,
                float* p1, float* p2) {
  TORCH_CHECK(!(p1 && o.skip.defined()), "conv k64: stats with skip");
  dim3 grid(cdiv(g.M, 128), g.Coutp / 128);
  auto s = at::cuda::getCurrentCUDAStream();
#define RTHD_K64_LAUNCH(SKIP_, STATS_)                                     \
  hipLaunchKernelGGL((conv_fwd_bf16_k64_kernel<SKIP_, STATS_>), grid,      \
      dim3(256), 2 * 32768, s, conv_ptr<const bf16>(o.x),                  \
      conv_ptr<const bf16>(o.wpk), o.scale.data_ptr<float>(),              \
      o.shift.data_ptr<float>(), conv_ptr<const bf16>(o.skip),             \
      zero_page_bf16(o.x), conv_ptr<bf16>(o.y), g, act, p1, p2)
  if (p1)                    RTHD_K64_LAUNCH(false, true);
  else if (o.skip.defined()) RTHD_K64_LAUNCH(true, false);
  else                       RTHD_K64_LAUNCH(false, false);
#undef RTHD_K64_LAUNCH
  HIP_CHECK_LAST();
}

torch::Tensor conv_fwd_k64(torch::Tensor x, torch::Tensor wpk,
                           torch::Tensor scale, torch::Tensor shift,
                           c10::optional<torch::Tensor> skip,
                           int64_t KH, int64_t KW, int64_t stride,
                           int64_t pad, int64_t Cout, int64_t act) {
  TORCH_CHECK(wpk.scalar_type() == at::kBFloat16,
              "conv_fwd_k64: bf16 packed weights required");
  const ConvGeo g = make_conv_geo("conv_fwd_k64", x, wpk, KH, KW, stride,
                                  pad, Cout, 64);
  auto o = prep_conv_operands(g, x, wpk, scale, shift, skip, at::kBFloat16,
                              at::kBFloat16);
  launch_k64(g, o, (int)act, nullptr, nullptr);
  return o.y;
}

}  // namespace rthd
