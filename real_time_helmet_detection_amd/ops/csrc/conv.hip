// Implicit-GEMM convolution for gfx950 MFMA, NHWC, with fused
// scale/shift(+bias)/activation(+residual-add) epilogue.
//
// GEMM view (guide §5 anatomy): M = B*Ho*Wo output pixels, N = Cout,
// K = KH*KW*Cin, tap-major. Each workgroup computes a BM=128 x BN=128
// output tile with 4 waves (2x2 of 64x64 wave tiles, 4x4 fragments of
// v_mfma_f32_16x16x32_bf16 / _16x16x4_f32). The K loop walks taps x
// 32-channel blocks; for each step the A tile (128 px x 32 ch) is gathered
// with zero-padding predication and the B tile (128 cout x 32 ch) is read
// from the pre-packed weight buffer, both staged in double-buffered LDS
// with an XOR slot swizzle (guide §6 G4) to keep ds_read_b128 conflict-low.
//
// Weights are pre-packed by pack_weights_* into [taps][Cout_pad][Cin_pad]
// (k contiguous per output-channel row) so A and B fragments use the SAME
// LDS image and read pattern. dgrad reuses this kernel with rotated,
// transposed packed weights (pack is done by the python wrapper calling
// pack_weights with swap=true).
//
// Requires Cin % 32 == 0 (every conv in the model except the 3-channel
// stem, which has its own kernel in stem.hip).
#include <mutex>
#include <type_traits>
#include <unordered_map>

#include "conv_common.h"

namespace rthd {

// ------------------------------ weight packing ------------------------------

// torch weight (Cout, Cin, KH, KW) fp32 -> packed [T][Coutp][Cinp] (T dtype)
// swap=false: pk[t][co][ci] = w[co][ci][t/KW][t%KW]
// swap=true (dgrad): roles swapped + taps rotated:
//   pk[t][ci][co] = w[co][ci][KH-1-t/KW][KW-1-t%KW]  (rows indexed by ci)
// reads w through explicit element strides so channels_last master
// weights pack WITHOUT a contiguous() relayout first (that copy ran
// twice per conv per training step — ~0.5 ms/step)

// the master weight as the pack kernels read it
struct PackSrc {
  const float* w;
  int Cout, Cin, KH, KW;
  int64_t s0, s1, s2, s3;
};

// element i of one packed image. Rows/Rp: row count (+pad) of pk (= Cout or
// Cin); Kp: padded k per tap
template <typename T>
DEV_INLINE void pack_weight_elem(const PackSrc& a, T* __restrict__ pk,
                                 int64_t i, int Rows, int Rp, int Kp,
                                 int swap) {
  const int t = i / ((int64_t)Rp * Kp);
  const int row = (i / Kp) % Rp;
  const int k = i % Kp;
  float v = 0.f;
  const int Kdim = swap ? a.Cout : a.Cin;
  if (row < Rows && k < Kdim) {
    int co, ci, ty, tx;
    if (!swap) {
      co = row; ci = k; ty = t / a.KW; tx = t % a.KW;
    } else {
      ci = row; co = k; ty = a.KH - 1 - t / a.KW; tx = a.KW - 1 - t % a.KW;
    }
    v = a.w[co * a.s0 + ci * a.s1 + ty * a.s2 + tx * a.s3];
  }
  stf(&pk[i], v);
}

template <typename T>
__global__ void pack_weights_kernel(const PackSrc a, T* __restrict__ pk,
                                    int Rows, int Rp, int Kp, int swap) {
  const int64_t n = (int64_t)a.KH * a.KW * Rp * Kp;
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) pack_weight_elem(a, pk, i, Rows, Rp, Kp, swap);
}

// both images of one weight in one launch: index range [0, nf) is the
// forward image (swap=false), [nf, nf + nd) the dgrad image (swap=true)
template <typename TF, typename TD>
__global__ void pack_weights_pair_kernel(const PackSrc a,
                                         TF* __restrict__ pk,
                                         TD* __restrict__ pkt, int Rpf,
                                         int Kpf, int Rpd, int Kpd) {
  const int64_t nf = (int64_t)a.KH * a.KW * Rpf * Kpf;
  const int64_t n = nf + (int64_t)a.KH * a.KW * Rpd * Kpd;
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    if (i < nf) pack_weight_elem(a, pk, i, a.Cout, Rpf, Kpf, 0);
    else pack_weight_elem(a, pkt, i - nf, a.Cin, Rpd, Kpd, 1);
  }
}

namespace {

// geometry of one packed image of wc
struct PackGeo {
  int Rows, Rp, Kp;
  int64_t n;
};

PackGeo pack_geo(const torch::Tensor& wc, bool swap) {
  const int Cout = wc.size(0), Cin = wc.size(1);
  const int T_ = wc.size(2) * wc.size(3);
  PackGeo g;
  g.Rows = swap ? Cin : Cout;
  const int Kdim = swap ? Cout : Cin;
  g.Rp = (int)cdiv(g.Rows, 128) * 128;
  // K pads to 64 so the 64-ch-per-step kernel variant shares the same
  // packed image as the 32-ch ones (pad region is zeros)
  g.Kp = (int)cdiv(Kdim, 64) * 64;
  g.n = (int64_t)T_ * g.Rp * g.Kp;
  return g;
}

PackSrc pack_src(const torch::Tensor& wc) {
  const auto ws = wc.strides();
  return {wc.data_ptr<float>(), (int)wc.size(0), (int)wc.size(1),
          (int)wc.size(2), (int)wc.size(3), ws[0], ws[1], ws[2], ws[3]};
}

torch::Tensor pack_alloc(const torch::Tensor& wc, const PackGeo& g,
                         bool to_bf16) {
  return torch::empty({wc.size(2) * wc.size(3), g.Rp, g.Kp},
      wc.options().dtype(to_bf16 ? at::kBFloat16 : at::kFloat));
}

}  // namespace

torch::Tensor pack_weights(torch::Tensor w, bool swap, bool to_bf16) {
  auto wc = w.to(at::kFloat);  // (Cout, Cin, KH, KW), any stride layout
  const PackGeo g = pack_geo(wc, swap);
  auto pk = pack_alloc(wc, g, to_bf16);
  auto s = at::cuda::getCurrentCUDAStream();
  if (to_bf16)
    hipLaunchKernelGGL((pack_weights_kernel<bf16>), dim3(ew_grid(g.n, 256)),
        dim3(256), 0, s, pack_src(wc),
        reinterpret_cast<bf16*>(pk.data_ptr()), g.Rows, g.Rp, g.Kp,
        swap ? 1 : 0);
  else
    hipLaunchKernelGGL((pack_weights_kernel<float>), dim3(ew_grid(g.n, 256)),
        dim3(256), 0, s, pack_src(wc), pk.data_ptr<float>(), g.Rows, g.Rp,
        g.Kp, swap ? 1 : 0);
  HIP_CHECK_LAST();
  return pk;
}

// (pack_weights(w, false, to_bf16_fwd), pack_weights(w, true, to_bf16_dgrad))
// from one launch: a training step needs both images of the same master
// weight, the second one on the backward's critical path
std::vector<torch::Tensor> pack_weights_pair(torch::Tensor w,
                                             bool to_bf16_fwd,
                                             bool to_bf16_dgrad) {
  auto wc = w.to(at::kFloat);
  const PackGeo gf = pack_geo(wc, false), gd = pack_geo(wc, true);
  auto pk = pack_alloc(wc, gf, to_bf16_fwd);
  auto pkt = pack_alloc(wc, gd, to_bf16_dgrad);
  auto s = at::cuda::getCurrentCUDAStream();
  const dim3 grid(ew_grid(gf.n + gd.n, 256));
  auto launch = [&](auto* pf, auto* pd) {
    using TF = std::remove_pointer_t<decltype(pf)>;
    using TD = std::remove_pointer_t<decltype(pd)>;
    hipLaunchKernelGGL((pack_weights_pair_kernel<TF, TD>), grid, dim3(256),
        0, s, pack_src(wc), pf, pd, gf.Rp, gf.Kp, gd.Rp, gd.Kp);
  };
  bf16* fb = reinterpret_cast<bf16*>(pk.data_ptr());
  bf16* db = reinterpret_cast<bf16*>(pkt.data_ptr());
  float* ff = reinterpret_cast<float*>(pk.data_ptr());
  float* df = reinterpret_cast<float*>(pkt.data_ptr());
  if (to_bf16_fwd && to_bf16_dgrad) launch(fb, db);
  else if (to_bf16_fwd) launch(fb, df);
  else if (to_bf16_dgrad) launch(ff, db);
  else launch(ff, df);
  HIP_CHECK_LAST();
  return {pk, pkt};
}

// ------------------------------ conv forward --------------------------------

// fp32 LDS tile: 128-B rows, element swizzle k' = k ^ (row & 15) within
// the row (the bf16 tile uses lds_off_row64 from conv_common.h).
DEV_INLINE int lds_off_f32(int row, int k) {
  return row * 128 + ((k ^ (row & 15)) << 2);
}

// act codes from common.h; epilogue: y = act(acc*scale[c] + shift[c] (+skip))
//
// Staging is ASYNC global->LDS (global_load_lds_dwordx4, guide G15): each
// K-step issues the NEXT step's 4 glds per thread into the alternate LDS
// buffer, then runs this step's fragment reads + MFMA; the barrier at the
// step end both publishes the prefetched tile and closes the read window —
// ONE barrier per K-step and no ds_write pass or staging VGPRs. Out-of-range
// pixels point their source at a 16-B zero page (glds cannot select-zero).
// The per-lane SOURCE k8 is pre-swizzled so the lane-linear LDS image equals
// the XOR-swizzled layout the fragment reads expect (guide rule 21).
// STATS: conv_epilogue's column partials go to sp1/sp2[2*gridDim.x][Cout],
// one row per (mblk, wave-row).
template <bool HAS_SKIP, bool STATS = false>
__global__ __launch_bounds__(256)
void conv_fwd_bf16_kernel(const bf16* __restrict__ x,
                          const bf16* __restrict__ wpk,
                          const float* __restrict__ scale,
                          const float* __restrict__ shift,
                          const bf16* __restrict__ skip,
                          const bf16* __restrict__ zpage,
                          bf16* __restrict__ y,
                          ConvGeo g, int act,
                          float* __restrict__ sp1 = nullptr,
                          float* __restrict__ sp2 = nullptr) {
  // grid: (M/128) x (Coutp/128); 4 waves (2x2 of 64x64).
  //
  // K loop = taps (outer) x 32-ch blocks (inner, incremental addressing —
  // the flat-step version spent ~116 VALU/step on 64-bit address chains).
  // Staging: async glds into a 3-deep LDS ring, TWO tiles in flight across
  // each barrier via counted `s_waitcnt vmcnt(4)` + raw s_barrier (guide §5
  // 'pipelining across barriers': a plain __syncthreads drains vmcnt(0) and
  // de-pipelines the span). OOB pixels source a 16-B zero page.
  const int mblk = blockIdx.x;
  const int nblk = blockIdx.y;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* lds = smem;  // 3 x (A 8KB | B 8KB)

  f32x4 acc[4][4] = {};

  const int st_row = tid >> 2;
  const int st_k8 = tid & 3;
  const int k8s0 = st_k8 ^ ((st_row >> 2) & 3);
  const int k8s1 = st_k8 ^ (((st_row + 64) >> 2) & 3);
  const int wbase = wid * 1024;

  // per-thread pixel decomposition for its two staged rows
  int am[2], ab[2], ay[2], ax[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    am[h] = mblk * 128 + st_row + 64 * h;
    pixel_decompose(am[h], g, &ab[h], &ay[h], &ax[h]);
  }

  const int kc = g.Cinp / 32;
  const int taps = g.KH * g.KW;
  const int nsteps = taps * kc;

  // stage issue state, advanced incrementally by issue_step()
  int is_step = 0;        // next step to issue
  int is_t = 0, is_kb = 0;
  const bf16* aptr[2];    // current tap's base source (or zpage)
  const bf16* bptr[2];
  bool avalid[2];
  auto tap_setup = [&]() {
    const int dy_ = is_t / g.KW - g.pad;
    const int dx_ = is_t % g.KW - g.pad;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int iy = ay[h] * g.stride + dy_;
      const int ix = ax[h] * g.stride + dx_;
      avalid[h] = am[h] < g.M && iy >= 0 && iy < g.H && ix >= 0 &&
                  ix < g.W;
      const int c0 = (h ? k8s1 : k8s0) * 8;
      aptr[h] = avalid[h]
          ? x + (((int64_t)ab[h] * g.H + iy) * g.W + ix) * g.Cin + c0
          : zpage;
    }
    bptr[0] = wpk + ((int64_t)is_t * g.Coutp + nblk * 128 + st_row) *
        g.Cinp + k8s0 * 8;
    bptr[1] = wpk + ((int64_t)is_t * g.Coutp + nblk * 128 + st_row + 64) *
        g.Cinp + k8s1 * 8;
  };
  tap_setup();

  auto issue_step = [&]() {
    char* base = lds + (is_step % 3) * 16384;
    const int cb = is_kb * 32;
    // channel-block bound (only non-trivial when Cin % 32 != 0)
    const bf16* a0 = (avalid[0] && cb + k8s0 * 8 < g.Cin) ? aptr[0] + cb
                                                          : zpage;
    const bf16* a1 = (avalid[1] && cb + k8s1 * 8 < g.Cin) ? aptr[1] + cb
                                                          : zpage;
    __builtin_amdgcn_global_load_lds((glb_void*)a0,
        (lds_void*)(base + wbase), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((glb_void*)a1,
        (lds_void*)(base + 4096 + wbase), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((glb_void*)(bptr[0] + cb),
        (lds_void*)(base + 8192 + wbase), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((glb_void*)(bptr[1] + cb),
        (lds_void*)(base + 12288 + wbase), 16, 0, 0);
    ++is_step;
    if (++is_kb == kc) {
      is_kb = 0;
      if (++is_t < taps) tap_setup();
    }
  };

  // prologue: two tiles in flight (count the wait to the FIRST tile)
  issue_step();
  if (nsteps > 1) {
    issue_step();
    asm volatile("s_waitcnt vmcnt(%0)" ::"i"(4) : "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(%0)" ::"i"(0) : "memory");
  }
  __builtin_amdgcn_s_barrier();

  for (int step = 0; step < nsteps; ++step) {
    char* A = lds + (step % 3) * 16384;
    char* B = A + 8192;
    if (step + 2 < nsteps) issue_step();

    const int arow_base = wr * 64 + (lane & 15);
    const int brow_base = wc * 64 + (lane & 15);
    const int k8 = lane >> 4;
    bf16x8 afrag[4], bfrag[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      afrag[i] = *reinterpret_cast<const bf16x8*>(
          A + lds_off_row64(arow_base + 16 * i, k8));
      bfrag[i] = *reinterpret_cast<const bf16x8*>(
          B + lds_off_row64(brow_base + 16 * i, k8));
    }
    // MFMA-phase issue priority (measured +6% on the wgrad kernel: the
    // co-resident waves still issuing staging yield slots to the MFMAs)
    asm volatile("s_setprio 1");
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            afrag[mi], bfrag[ni], acc[mi][ni], 0, 0, 0);
    asm volatile("s_setprio 0");

    // wait for step+1's tile (leave step+2's 4 glds in flight), then a raw
    // barrier — every wave has passed its own counted wait, so the tile is
    // complete before any wave reads it.
    if (step + 2 < nsteps + 1) {
      if (step + 2 < nsteps)
        asm volatile("s_waitcnt vmcnt(%0)" ::"i"(4) : "memory");
      else
        asm volatile("s_waitcnt vmcnt(%0)" ::"i"(0) : "memory");
    }
    __builtin_amdgcn_s_barrier();
  }

  // stats partial row: chunk = mblk*2 + wr
  conv_epilogue<4, 4, HAS_SKIP, STATS>(
      acc, mblk * 128 + wr * 64, nblk * 128 + wc * 64 + (lane & 15), lane,
      g.M, g.Cout, scale, shift, skip, y, act, sp1, sp2,
      (int64_t)mblk * 2 + wr);
}

// fp32-exact variant: v_mfma_f32_16x16x4_f32, one A/B float per lane
template <bool HAS_SKIP>
__global__ __launch_bounds__(256)
void conv_fwd_f32_kernel(const float* __restrict__ x,
                         const float* __restrict__ wpk,
                         const float* __restrict__ scale,
                         const float* __restrict__ shift,
                         const float* __restrict__ skip,
                         float* __restrict__ y,
                         ConvGeo g, int act) {
  const int mblk = blockIdx.x;
  const int nblk = blockIdx.y;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* ldsA = reinterpret_cast<float*>(smem);            // 16 KB
  float* ldsB = reinterpret_cast<float*>(smem + 16384);    // 16 KB

  f32x4 acc[4][4] = {};

  // A tile rows are 32 floats (128 B); each thread stages 2 rows x 8 floats
  const int st_row = tid >> 2;
  const int st_k8 = (tid & 3) * 8;

  int am[2], ab[2], ayy[2], axx[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    am[h] = mblk * 128 + st_row + 64 * h;
    pixel_decompose(am[h], g, &ab[h], &ayy[h], &axx[h]);
  }

  const int nsteps = g.KH * g.KW * (g.Cinp / 32);
  const int kc_per_tap = g.Cinp / 32;

  for (int step = 0; step < nsteps; ++step) {
    const int t = step / kc_per_tap;
    const int kb = step % kc_per_tap;
    const int dy = t / g.KW - g.pad;
    const int dx = t % g.KW - g.pad;
    float* A = ldsA;
    float* B = ldsB;
    __syncthreads();  // previous step's reads done before overwrite

#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int iy = ayy[h] * g.stride + dy;
      const int ix = axx[h] * g.stride + dx;
      const int c0 = kb * 32 + st_k8;
      float v[8] = {};
      if (am[h] < g.M && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W &&
          c0 < g.Cin) {
        const float* src =
            x + (((int64_t)ab[h] * g.H + iy) * g.W + ix) * g.Cin + c0;
#pragma unroll
        for (int e = 0; e < 8; ++e)
          v[e] = (c0 + e < g.Cin) ? src[e] : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        *reinterpret_cast<float*>(
            reinterpret_cast<char*>(A) +
            lds_off_f32(st_row + 64 * h, st_k8 + e)) = v[e];
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = st_row + 64 * h;
      const int64_t src_off =
          ((int64_t)t * g.Coutp + nblk * 128 + row) * g.Cinp + kb * 32 +
          st_k8;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        *reinterpret_cast<float*>(
            reinterpret_cast<char*>(B) + lds_off_f32(row, st_k8 + e)) =
            wpk[src_off + e];
      }
    }

    __syncthreads();

    const int arow = wr * 64 + (lane & 15);
    const int brow = wc * 64 + (lane & 15);
    const int kl = lane >> 4;  // 0..3
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {  // 8 x K=4 = 32
      float afrag[4], bfrag[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        afrag[i] = *reinterpret_cast<const float*>(
            reinterpret_cast<char*>(A) +
            lds_off_f32(arow + 16 * i, ks * 4 + kl));
        bfrag[i] = *reinterpret_cast<const float*>(
            reinterpret_cast<char*>(B) +
            lds_off_f32(brow + 16 * i, ks * 4 + kl));
      }
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(
              afrag[mi], bfrag[ni], acc[mi][ni], 0, 0, 0);
    }

    __syncthreads();
  }

  conv_epilogue<4, 4, HAS_SKIP, false>(
      acc, mblk * 128 + wr * 64, nblk * 128 + wc * 64 + (lane & 15), lane,
      g.M, g.Cout, scale, shift, skip, y, act, nullptr, nullptr, 0);
}

// ---------------------------- autotune cache --------------------------------
// cudnn.benchmark analog (SURVEY.md §2.3 last row): per (shape, dtype) the
// first eligible call MEASURES the 128x128 kernel against the 64x64
// (+split-K) variants on the current stream and caches the winner; under
// stream capture (hipGraph) or RTHD_NO_AUTOTUNE an unseen shape takes the
// fill-based heuristic instead (no timing APIs are capture-legal).

// per-device cached 16-B zero page for the glds out-of-range source (a
// fresh torch::zeros({8}) per conv call was ~85 FillFunctor launches per
// training step). First use happens during eager warmup (never inside a
// graph capture), so the allocation is from the regular allocator pool.
const bf16* zero_page_bf16(const torch::Tensor& like) {
  static std::mutex mu;
  static std::unordered_map<int, torch::Tensor> pages;
  const int dev = like.device().index();
  std::lock_guard<std::mutex> lk(mu);
  auto it = pages.find(dev);
  if (it == pages.end())
    it = pages.emplace(dev, torch::zeros({8},
        like.options().dtype(at::kBFloat16))).first;
  return reinterpret_cast<const bf16*>(it->second.data_ptr());
}

namespace {

// variants: 0 = the 128x128/K32 kernel of this file, 1 = 64x64 split-K
// (small spatial / Cout<=64 fill), 2 = 128x128/K64 double-buffer (fewer
// barriers+glds issues per channel), 3 = halo-tile 3x3 (conv_halo.hip; its
// stats epilogue needs Cout % 8 == 0: conv_fwd_stats otherwise runs `alt`,
// the faster of 0/2)
struct ConvChoice { int small; int splitk; int alt = 0; };

std::mutex g_conv_tune_mu;
std::unordered_map<uint64_t, ConvChoice> g_conv_tune;

uint64_t conv_key(const ConvGeo& g) {
  uint64_t h = 1469598103934665603ull;
  auto mix = [&h](uint64_t v) {
    h ^= v + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2);
  };
  mix(g.M); mix(g.Cin); mix(g.Cout); mix(g.KH); mix(g.KW); mix(g.stride);
  // M does not fix H, W or pad, which decide whether the halo variant may
  // be a shape's cached choice
  mix(halo_eligible(g));
  return h;
}

// 128x128/K32 bf16 kernel on prepared operands; p1/p2 (both or neither,
// no skip) select the fused-stats epilogue
void launch_big(const ConvGeo& g, const ConvOperands& o, int act,
                float* p1, float* p2) {
  TORCH_CHECK(!(p1 && o.skip.defined()), "conv big: stats with skip");
  dim3 grid(cdiv(g.M, 128), g.Coutp / 128);
  auto s = at::cuda::getCurrentCUDAStream();
#define RTHD_BIG_LAUNCH(SKIP_, STATS_)                                     \
  hipLaunchKernelGGL((conv_fwd_bf16_kernel<SKIP_, STATS_>), grid,          \
      dim3(256), 3 * 16384, s, conv_ptr<const bf16>(o.x),                  \
      conv_ptr<const bf16>(o.wpk), o.scale.data_ptr<float>(),              \
      o.shift.data_ptr<float>(), conv_ptr<const bf16>(o.skip),             \
      zero_page_bf16(o.x), conv_ptr<bf16>(o.y), g, act, p1, p2)
  if (p1)                    RTHD_BIG_LAUNCH(false, true);
  else if (o.skip.defined()) RTHD_BIG_LAUNCH(true, false);
  else                       RTHD_BIG_LAUNCH(false, false);
#undef RTHD_BIG_LAUNCH
  HIP_CHECK_LAST();
}

// per-shape bf16 variant: the cached choice, else (first sight of the
// shape) the heuristic or a measurement, cached once decided
ConvChoice choose_conv_variant(const ConvGeo& g, const ConvOperands& o,
                               int act) {
  const uint64_t key = conv_key(g);
  {
    std::lock_guard<std::mutex> lk(g_conv_tune_mu);
    auto it = g_conv_tune.find(key);
    if (it != g_conv_tune.end()) return it->second;
  }
  // split-K candidates only where fill is the problem
  const int big_blocks = (int)cdiv(g.M, 128) * (g.Coutp / 128);
  const int nsteps = g.KH * g.KW * (g.Cinp / 32);
  const int base64 = (int)cdiv(g.M, 64) * (int)cdiv(g.Cout, 64);
  std::vector<int> cands;
  if (big_blocks < 512 || g.Cout <= 64) {
    for (int sk : {1, 2, 4, 8, 16}) {
      if (sk > 1 && (nsteps + sk - 1) / sk < 2) break;
      if ((int64_t)base64 * sk > 16384) break;
      cands.push_back(sk);
    }
  }
  ConvChoice ch{0, 1};
  auto s = at::cuda::getCurrentCUDAStream();
  if (stream_capturing(s) || getenv("RTHD_NO_AUTOTUNE")) {
    if (big_blocks >= 512 && g.Cout > 64) {
      // the halo variant measured ahead of both 128-tile kernels on every
      // eligible shape of this size (profiles/conv_halo.md)
      if (halo_eligible(g)) ch = {3, 1, 0};
      else                  ch = {0, 1};
    } else if (!cands.empty()) {
      ch = {1, cands.back()};
      for (int sk : cands) {
        if (base64 * sk >= 768) { ch = {1, sk}; break; }
      }
    }
  } else {
    float best = time_usec(
        [&] { launch_big(g, o, act, nullptr, nullptr); }, s.stream());
    const float tk = time_usec(
        [&] { launch_k64(g, o, act, nullptr, nullptr); }, s.stream());
    if (tk < best) { best = tk; ch = {2, 1}; }
    const int alt = ch.small;
    for (int sk : cands) {
      const float t = time_usec(
          [&] { launch_small(g, o, act, sk); }, s.stream());
      if (t < best) { best = t; ch = {1, sk}; }
    }
    if (halo_eligible(g)) {
      const float t = time_usec([&] { launch_halo(g, o, act); }, s.stream());
      if (t < best) { best = t; ch = {3, 1, alt}; }
    }
  }
  std::lock_guard<std::mutex> lk(g_conv_tune_mu);
  g_conv_tune[key] = ch;
  return ch;
}

}  // namespace

// host wrapper; x NCHW-logical channels_last; wpk from pack_weights.
torch::Tensor conv_fwd(torch::Tensor x, torch::Tensor wpk,
                       torch::Tensor scale, torch::Tensor shift,
                       c10::optional<torch::Tensor> skip,
                       int64_t KH, int64_t KW, int64_t stride, int64_t pad,
                       int64_t Cout, int64_t act) {
  const bool bf16_mode = wpk.scalar_type() == at::kBFloat16;
  TORCH_CHECK(bf16_mode || x.scalar_type() == at::kFloat,
              "f32 conv needs f32 input");
  const ConvGeo g = make_conv_geo("conv_fwd", x, wpk, KH, KW, stride, pad,
                                  Cout, 64);
  const auto dtype = bf16_mode ? at::kBFloat16 : at::kFloat;
  auto o = prep_conv_operands(g, x, wpk, scale, shift, skip, dtype, dtype);

  if (bf16_mode) {
    const ConvChoice ch = choose_conv_variant(g, o, (int)act);
    if (ch.small == 1)      launch_small(g, o, (int)act, ch.splitk);
    else if (ch.small == 2) launch_k64(g, o, (int)act, nullptr, nullptr);
    else if (ch.small == 3) launch_halo(g, o, (int)act);
    else                    launch_big(g, o, (int)act, nullptr, nullptr);
    return o.y;
  }

  dim3 grid(cdiv(g.M, 128), g.Coutp / 128);
  auto s = at::cuda::getCurrentCUDAStream();
  if (o.skip.defined())
    hipLaunchKernelGGL((conv_fwd_f32_kernel<true>), grid, dim3(256), 32768,
        s, o.x.data_ptr<float>(), wpk.data_ptr<float>(),
        o.scale.data_ptr<float>(), o.shift.data_ptr<float>(),
        o.skip.data_ptr<float>(), o.y.data_ptr<float>(), g, (int)act);
  else
    hipLaunchKernelGGL((conv_fwd_f32_kernel<false>), grid, dim3(256), 32768,
        s, o.x.data_ptr<float>(), wpk.data_ptr<float>(),
        o.scale.data_ptr<float>(), o.shift.data_ptr<float>(),
        (const float*)nullptr, o.y.data_ptr<float>(), g, (int)act);
  HIP_CHECK_LAST();
  return o.y;
}

// ---------------------- training-BN fused-stats forward ---------------------
// y = act(conv*scale + shift) PLUS the per-column sum/sumsq partials the
// BN stats need — saves the standalone colsum pass over y. Returns
// {y, p1, p2}; p1/p2 are fp32 [rows, Cout] partial rows that
// bn_stats_from_parts reduces in fixed order (deterministic): one row per
// 8x16 tile from the halo kernel, 2*Mblks rows from the 128-tile kernels.
// Returns {y} where the shape's variant has no stats epilogue (split-K) or
// the caller's rule declines it; the caller then runs bn_stats.
//
// halo_min_tiles < 0: every variant with a stats epilogue uses it (the
// RTHD_FUSED_STATS=1 meaning). halo_min_tiles >= 0: only the halo kernel
// does, and only on shapes of at least that many tiles — the 128-tile
// kernels' stats epilogue is a measured loss, and below the threshold the
// colsum pass is launch-bound and the finish launch costs as much
// (profiles/bn_passes.md). Any other shape runs its plain variant.
std::vector<torch::Tensor> conv_fwd_stats(
    torch::Tensor x, torch::Tensor wpk, torch::Tensor scale,
    torch::Tensor shift, int64_t KH, int64_t KW, int64_t stride,
    int64_t pad, int64_t Cout, int64_t act, int64_t halo_min_tiles) {
  TORCH_CHECK(wpk.scalar_type() == at::kBFloat16,
              "conv_fwd_stats: bf16 only (f32 path uses bn_stats)");
  const ConvGeo g = make_conv_geo("conv_fwd_stats", x, wpk, KH, KW, stride,
                                  pad, Cout, 64);
  auto o = prep_conv_operands(g, x, wpk, scale, shift, c10::nullopt,
                              at::kBFloat16, at::kBFloat16);
  const ConvChoice ch = choose_conv_variant(g, o, (int)act);
  const auto fopt = o.x.options().dtype(at::kFloat);
  if (ch.small == 3 && halo_stats_ok(g) &&
      halo_stats_rows(g) >= halo_min_tiles) {
    auto p1 = torch::empty({halo_stats_rows(g), Cout}, fopt);
    auto p2 = torch::empty_like(p1);
    launch_halo_stats(g, o, (int)act, p1.data_ptr<float>(),
                      p2.data_ptr<float>(), (int)Cout);
    return {o.y, p1, p2};
  }
  if (halo_min_tiles >= 0) {
    if (ch.small == 1)      launch_small(g, o, (int)act, ch.splitk);
    else if (ch.small == 2) launch_k64(g, o, (int)act, nullptr, nullptr);
    else if (ch.small == 3) launch_halo(g, o, (int)act);
    else                    launch_big(g, o, (int)act, nullptr, nullptr);
    return {o.y};
  }
  if (ch.small == 1) {
    // split-K variant has no stats epilogue — caller runs bn_stats
    launch_small(g, o, (int)act, ch.splitk);
    return {o.y};
  }
  auto p1 = torch::empty({2 * cdiv(g.M, 128), Cout}, fopt);
  auto p2 = torch::empty_like(p1);
  // a halo shape whose Cout has no wide epilogue keeps the faster of the
  // two 128-tile kernels here
  const int variant = ch.small == 3 ? ch.alt : ch.small;
  if (variant == 2)
    launch_k64(g, o, (int)act, p1.data_ptr<float>(), p2.data_ptr<float>());
  else
    launch_big(g, o, (int)act, p1.data_ptr<float>(), p2.data_ptr<float>());
  return {o.y, p1, p2};
}

}  // namespace rthd
