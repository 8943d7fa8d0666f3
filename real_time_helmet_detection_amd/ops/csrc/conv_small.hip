// Small-spatial implicit-GEMM conv variant for gfx950: BM=BN=64 tiles with
// optional split-K, for the hourglass levels where M = B*Ho*Wo is too small
// to fill 256 CUs with 128x128 tiles (8^2: 8 blocks, 16^2: 32 blocks — the
// round-1 profile's 9.4 TF @8^2 launch/fill-bound hole; SURVEY.md §2.3
// autotune row). Split-K slices the tap x channel-block K loop across
// gridDim.z blocks that write fp32 partials; a fixed-order reduce kernel
// applies the scale/shift/act(+skip) epilogue — same deterministic-partials
// pattern the wgrad kernel proved.
//
// Tiling: 4 waves as 2x2 of 32x32 wave tiles (2x2 fragments of
// v_mfma_f32_16x16x32_bf16). Staging mirrors conv.hip: async
// global_load_lds into a 3-deep LDS ring (24 KB), two tiles in flight
// across counted s_waitcnt vmcnt barriers, sources pre-swizzled so the
// lane-linear glds image equals the XOR-swizzled layout the fragment
// ds_read_b128s expect. bf16 only — the f32-exact path keeps the 128x128
// kernel (fill is not its bottleneck in the fp32 engine).
#include "conv_common.h"

namespace rthd {

// SPLIT=true: write fp32 partials to part[z][M][Coutp64] (no epilogue).
// SPLIT=false: fused scale/shift/act(+skip) epilogue straight to y.
template <bool SPLIT, bool HAS_SKIP>
__global__ __launch_bounds__(256)
void conv_fwd_bf16_64_kernel(const bf16* __restrict__ x,
                             const bf16* __restrict__ wpk,
                             const float* __restrict__ scale,
                             const float* __restrict__ shift,
                             const bf16* __restrict__ skip,
                             const bf16* __restrict__ zpage,
                             bf16* __restrict__ y,
                             float* __restrict__ part, int Coutp64,
                             ConvGeo g, int ksteps, int kchunk, int act) {
  // ksteps = taps * Cinp/32 in all; kchunk = K steps per z-block (split-K)
  const int mblk = blockIdx.x;
  const int nblk = blockIdx.y;
  const int z = blockIdx.z;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* lds = smem;  // 3 x (A 4KB | B 4KB)

  f32x4 acc[2][2] = {};

  const int st_row = tid >> 2;
  const int st_k8 = tid & 3;
  const int k8s = st_k8 ^ ((st_row >> 2) & 3);
  const int wbase = wid * 1024;

  const int am = mblk * 64 + st_row;
  int ab, ay, ax;
  pixel_decompose(am, g, &ab, &ay, &ax);

  const int kc = g.Cinp / 32;
  const int taps = g.KH * g.KW;
  const int s0 = z * kchunk;
  int s1 = s0 + kchunk;
  if (s1 > ksteps) s1 = ksteps;
  const int nsteps = s1 - s0;
  if (nsteps <= 0) return;  // ragged last z-block

  int is_step = 0;
  int is_t = s0 / kc, is_kb = s0 % kc;
  const bf16* aptr;
  const bf16* bptr;
  bool avalid;
  auto tap_setup = [&]() {
    const int dy_ = is_t / g.KW - g.pad;
    const int dx_ = is_t % g.KW - g.pad;
    const int iy = ay * g.stride + dy_;
    const int ix = ax * g.stride + dx_;
    avalid = am < g.M && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W;
    aptr = avalid
        ? x + (((int64_t)ab * g.H + iy) * g.W + ix) * g.Cin + k8s * 8
        : zpage;
    bptr = wpk + ((int64_t)is_t * g.Coutp + nblk * 64 + st_row) * g.Cinp +
        k8s * 8;
  };
  tap_setup();

  auto issue_step = [&]() {
    char* base = lds + (is_step % 3) * 8192;
    const int cb = is_kb * 32;
    const bf16* a0 = (avalid && cb + k8s * 8 < g.Cin) ? aptr + cb : zpage;
    __builtin_amdgcn_global_load_lds((glb_void*)a0,
        (lds_void*)(base + wbase), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((glb_void*)(bptr + cb),
        (lds_void*)(base + 4096 + wbase), 16, 0, 0);
    ++is_step;
    if (++is_kb == kc) {
      is_kb = 0;
      if (++is_t < taps) tap_setup();
    }
  };

  issue_step();
  if (nsteps > 1) {
    issue_step();
    asm volatile("s_waitcnt vmcnt(%0)" ::"i"(2) : "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(%0)" ::"i"(0) : "memory");
  }
  __builtin_amdgcn_s_barrier();

  for (int step = 0; step < nsteps; ++step) {
    char* A = lds + (step % 3) * 8192;
    char* B = A + 4096;
    if (step + 2 < nsteps) issue_step();

    const int arow_base = wr * 32 + (lane & 15);
    const int brow_base = wc * 32 + (lane & 15);
    const int k8 = lane >> 4;
    bf16x8 afrag[2], bfrag[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      afrag[i] = *reinterpret_cast<const bf16x8*>(
          A + lds_off_row64(arow_base + 16 * i, k8));
      bfrag[i] = *reinterpret_cast<const bf16x8*>(
          B + lds_off_row64(brow_base + 16 * i, k8));
    }
    asm volatile("s_setprio 1");
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            afrag[mi], bfrag[ni], acc[mi][ni], 0, 0, 0);
    asm volatile("s_setprio 0");

    if (step + 2 < nsteps + 1) {
      if (step + 2 < nsteps)
        asm volatile("s_waitcnt vmcnt(%0)" ::"i"(2) : "memory");
      else
        asm volatile("s_waitcnt vmcnt(%0)" ::"i"(0) : "memory");
    }
    __builtin_amdgcn_s_barrier();
  }

  // ---- output ----
  const int col0 = nblk * 64 + wc * 32 + (lane & 15);
  const int row_in_frag = (lane >> 4) * 4;
  if (SPLIT) {
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = mblk * 64 + wr * 32 + mi * 16 + row_in_frag + r;
        if (m >= g.M) continue;
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
          const int c = col0 + ni * 16;
          part[((int64_t)z * g.M + m) * Coutp64 + c] = acc[mi][ni][r];
        }
      }
    }
  } else {
    conv_epilogue<2, 2, HAS_SKIP, false>(
        acc, mblk * 64 + wr * 32, col0, lane, g.M, g.Cout, scale, shift,
        skip, y, act, nullptr, nullptr, 0);
  }
}

// fixed-order sum over the SK partials + fused epilogue
template <bool HAS_SKIP>
__global__ void conv_splitk_reduce_kernel(const float* __restrict__ part,
                                          const float* __restrict__ scale,
                                          const float* __restrict__ shift,
                                          const bf16* __restrict__ skip,
                                          bf16* __restrict__ y,
                                          int SK, int Coutp64, int Cout,
                                          int64_t M, int act) {
  const int64_t n = M * Cout;
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int64_t m = i / Cout;
    const int c = (int)(i % Cout);
    float v = 0.f;
    for (int z = 0; z < SK; ++z)
      v += part[((int64_t)z * M + m) * Coutp64 + c];
    v = v * scale[c] + shift[c];
    if (HAS_SKIP) v += ldf(&skip[i]);
    v = apply_act(v, act);
    stf(&y[i], v);
  }
}

// BM=BN=64 (+split-K) path on prepared bf16 operands
void launch_small(const ConvGeo& g, const ConvOperands& o, int act,
                  int splitk) {
  const int ksteps = g.KH * g.KW * (g.Cinp / 32);
  int SK = splitk;
  if (SK < 1) SK = 1;
  if (SK > ksteps) SK = ksteps;
  const int kchunk = (int)cdiv(ksteps, SK);
  SK = (int)cdiv(ksteps, kchunk);  // drop empty z-blocks

  const bool has_skip = o.skip.defined();
  const int nblkN = (int)cdiv(g.Cout, 64);
  const int Coutp64 = nblkN * 64;
  dim3 grid(cdiv(g.M, 64), nblkN, SK);
  auto s = at::cuda::getCurrentCUDAStream();
  const size_t lds = 3 * 8192;

  auto* px = conv_ptr<const bf16>(o.x);
  auto* pw = conv_ptr<const bf16>(o.wpk);
  auto* py = conv_ptr<bf16>(o.y);
  const bf16* pz = zero_page_bf16(o.x);
  auto* ps = conv_ptr<const bf16>(o.skip);
  const float* sc = o.scale.data_ptr<float>();
  const float* sh = o.shift.data_ptr<float>();

  if (SK == 1) {
    if (has_skip)
      hipLaunchKernelGGL((conv_fwd_bf16_64_kernel<false, true>), grid,
          dim3(256), lds, s, px, pw, sc, sh, ps, pz, py, nullptr, Coutp64,
          g, ksteps, kchunk, act);
    else
      hipLaunchKernelGGL((conv_fwd_bf16_64_kernel<false, false>), grid,
          dim3(256), lds, s, px, pw, sc, sh, ps, pz, py, nullptr, Coutp64,
          g, ksteps, kchunk, act);
  } else {
    auto part = torch::empty({(int64_t)SK * g.M * Coutp64},
                             o.x.options().dtype(at::kFloat));
    hipLaunchKernelGGL((conv_fwd_bf16_64_kernel<true, false>), grid,
        dim3(256), lds, s, px, pw, sc, sh, nullptr, pz, py,
        part.data_ptr<float>(), Coutp64, g, ksteps, kchunk, act);
    const int64_t n = (int64_t)g.M * g.Cout;
    if (has_skip)
      hipLaunchKernelGGL((conv_splitk_reduce_kernel<true>),
          dim3(ew_grid(n, 256)), dim3(256), 0, s, part.data_ptr<float>(),
          sc, sh, ps, py, SK, Coutp64, g.Cout, (int64_t)g.M, act);
    else
      hipLaunchKernelGGL((conv_splitk_reduce_kernel<false>),
          dim3(ew_grid(n, 256)), dim3(256), 0, s, part.data_ptr<float>(),
          sc, sh, ps, py, SK, Coutp64, g.Cout, (int64_t)g.M, act);
  }
  HIP_CHECK_LAST();
}

torch::Tensor conv_fwd_small(torch::Tensor x, torch::Tensor wpk,
                             torch::Tensor scale, torch::Tensor shift,
                             c10::optional<torch::Tensor> skip,
                             int64_t KH, int64_t KW, int64_t stride,
                             int64_t pad, int64_t Cout, int64_t act,
                             int64_t splitk) {
  TORCH_CHECK(wpk.scalar_type() == at::kBFloat16,
              "conv_fwd_small: bf16 packed weights required");
  const ConvGeo g = make_conv_geo("conv_fwd_small", x, wpk, KH, KW, stride,
                                  pad, Cout, 64);
  auto o = prep_conv_operands(g, x, wpk, scale, shift, skip, at::kBFloat16,
                              at::kBFloat16);
  launch_small(g, o, (int)act, (int)splitk);
  return o.y;
}

}  // namespace rthd
