// bf16 wgrad on async LDS staging and transposed LDS reads.
//
// dW_t[tap][ci][co] = sum_px X[px+tap][ci] * dY[px][co] with the pixel dim
// as K of both operands. NHWC memory has channels contiguous, so the
// register-transpose kernel (wgrad_fast.hip) rebuilds [ch][px] images with
// VALU work between two barriers. Here the LDS image stays in memory order
// [px][ch]: it is filled by global_load_lds (no load passes through a VGPR,
// out-of-range sources are the 16-B zero page) and gfx950's
// ds_read_b64_tr_b16 delivers the fragments K-major on the read.
//
// - K-step = 64 px (two 16x16x32 k-blocks) in a 3-deep LDS ring: two steps
//   of loads are in flight across each barrier (counted s_waitcnt vmcnt +
//   one raw barrier per step), as in the K32 ring of conv.hip.
// - 4 waves as 2 (ci) x 2 (co); block tile 64 ci x 128 co, so a wave tile
//   of 32x64, 0.75 KB of fragment reads per MFMA and 72 KB of LDS = 2
//   blocks per CU (the 32x32 wave tile of the register-transpose kernel
//   needs 1 KB and saturates the LDS array).
// - One block per (tap, px-chunk, ci-tile, co-tile) cell as in
//   wgrad_fast.hip, on a 1-D grid whose block -> cell map keeps the blocks
//   that share a px chunk on one XCD (see the kernel).
// - The chunks, the k-slot of every pixel (slot (g,j) of k-block ks is px
//   32*ks + 8*g + j), the per-chunk fp32 partials and their fixed-order
//   reduce are those of wgrad_fast.hip: with equal chunk length the result
//   is bitwise equal to that kernel.
// The LDS layout, lane maps and source map live in wgrad_tr_geo.h and are
// walked on the host by tests/test_geo_checks.py.
#include "lds_async.h"
#include "wgrad_tr_geo.h"

namespace rthd {

namespace {

typedef __attribute__((address_space(3))) i16x4 lds_i16x4;

constexpr int WTR_NBUF = 3;   // LDS ring depth

// the two transposed reads of one 16x16x32 operand, k-slots 0..3 and 4..7,
// through the compiler builtin (the self-test; the main loop issues the
// same instruction through lds_read_tr16_b64)
DEV_INLINE bf16x8 tr_read_frag(const char* p0, const char* p1) {
  const i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4*)p0);
  const i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4*)p1);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// Lane-map self-check: a plain [32][64] image holding row*64+col, read as
// the 16x16x32 operand of each of the four 16-column blocks.
// out[cb][lane][j] must be (8*(lane>>4) + j)*64 + 16*cb + (lane&15).
__global__ __launch_bounds__(64)
void lds_tr16_selftest_kernel(short* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) short img[32 * 64];
  const int lane = threadIdx.x;
  for (int i = lane; i < 32 * 64; i += 64) img[i] = (short)i;
  __syncthreads();
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const char* base = reinterpret_cast<const char*>(img);
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    const int a0 = ((8 * g + q) * 64 + 16 * cb + 4 * p) * 2;
    const bf16x8 v = tr_read_frag(base + a0, base + a0 + 4 * 64 * 2);
    *reinterpret_cast<bf16x8*>(out + (cb * 64 + lane) * 8) = v;
  }
}

// wgrad_tr_kernel reads its fragments with lds_read_tr16_b64 and waits of
// its own: the audit rule of lds_async.h applies to every edit.
template <int BM, int BN>
__global__ __launch_bounds__(256)
void wgrad_tr_kernel(const bf16* __restrict__ x, const bf16* __restrict__ dy,
                     const bf16* __restrict__ zpage, float* __restrict__ dw,
                     WtrGeo g, int xcd_remap) {
  constexpr int MI = BM / 32, NI = BN / 32;   // 16-wide fragments per wave
  constexpr int XB = WTR_KB * BM * 2;         // bytes of the X tile
  constexpr int YB = WTR_KB * BN * 2;
  constexpr int STAGE = XB + YB;
  constexpr int NX = XB / 4096;               // glds per thread per step
  constexpr int NY = YB / 4096;
  constexpr int KS = WTR_KB / 32;             // MFMA k-blocks per step
  constexpr int RD1 = 2 * (MI + NI);          // fragment reads per k-block
  static_assert(KS == 2, "the fragment reads below are written for KS = 2");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  // One block per (tap, px-chunk, ci-tile, co-tile) cell, chunk-major: the
  // taps x tiles blocks that share one px chunk's X/dY data have
  // consecutive cell ids. With cell = block id those blocks land on all 8
  // XCDs and every XCD's L2 streams every chunk: 8x the unique bytes over
  // the fabric, which is what bounded the kernel (the loads ran at
  // Infinity-Cache bandwidth). With xcd_cell_remap (wgrad_tr_geo.h) a chunk
  // is fetched by one L2. Speed only: any placement computes the same bits.
  const int taps = g.KH * g.KW;
  const int ci_t = (g.Cin + BM - 1) / BM, co_t = (g.Cout + BN - 1) / BN;
  int cell = blockIdx.x;
  if (xcd_remap) cell = xcd_cell_remap(cell, gridDim.x);
  const int z = cell / (ci_t * co_t);
  const int t = z % taps;
  const int chunk = z / taps;
  const int ci0 = (cell % ci_t) * BM;
  const int co0 = (cell / ci_t % co_t) * BN;
  const int dyt = t / g.KW - g.pad;
  const int dxt = t % g.KW - g.pad;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;

  const int px_start = chunk * g.chunk_len;
  const int px_end = min(px_start + g.chunk_len, g.M);
  const int nsteps = (px_end - px_start + WTR_KB - 1) / WTR_KB;

  // staging slots of this lane: glds i of wave w is wave-instruction
  // f = 4i + w of the tile (wtr_stage_slot)
  WtrPix pix[NX];
  int xrow[NX], xch[NX], yrow[NY], ych[NY];
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    int c;
    wtr_stage_slot(i * 4 + wid, lane, BM, &xrow[i], &c);
    xch[i] = ci0 + c * 8;
    wtr_pix_init(px_start + xrow[i], g.Ho, g.Wo, &pix[i]);
  }
#pragma unroll
  for (int i = 0; i < NY; ++i) {
    int c;
    wtr_stage_slot(i * 4 + wid, lane, BN, &yrow[i], &c);
    ych[i] = co0 + c * 8;
  }
  const int adv_b = WTR_KB / (g.Ho * g.Wo);
  const int adv_q = WTR_KB % (g.Ho * g.Wo) / g.Wo, adv_r = WTR_KB % g.Wo;

  // issue the loads of K-step `step` into ring buffer `buf`
  auto issue_step = [&](int step, int buf) {
    char* base = smem + buf * STAGE;
    const int p0 = px_start + step * WTR_KB;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int64_t off = wtr_x_src(g, pix[i], p0 + xrow[i], px_end, dyt,
                                    dxt, xch[i]);
      const bf16* src = off < 0 ? zpage : x + off;
      __builtin_amdgcn_global_load_lds((glb_void*)src,
          (lds_void*)(base + wtr_stage_byte(i * 4 + wid, lane)), 16, 0, 0);
      wtr_pix_advance(&pix[i], adv_b, adv_q, adv_r, g.Ho, g.Wo);
    }
#pragma unroll
    for (int i = 0; i < NY; ++i) {
      const int64_t off = wtr_dy_src(g, p0 + yrow[i], px_end, ych[i]);
      const bf16* src = off < 0 ? zpage : dy + off;
      __builtin_amdgcn_global_load_lds((glb_void*)src,
          (lds_void*)(base + XB + wtr_stage_byte(i * 4 + wid, lane)),
          16, 0, 0);
    }
  };

  // fragment read addresses of k-block 0 in ring buffer 0 (k-block 1 is 32
  // rows further: an offset immediate)
  const uint32_t lds0 = lds_base(smem);
  uint32_t aoff[MI][2], boff[NI][2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
      aoff[mi][h] = lds0 + wtr_tr_addr(wr * MI + mi, 0, h, lane, BM);
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
      boff[ni][h] = lds0 + XB + wtr_tr_addr(wc * NI + ni, 0, h, lane, BN);
  }

  f32x4 acc[MI][NI] = {};

  // 3-deep ring, two K-steps of loads in flight across each barrier: the
  // loads of step s+2 are issued in step s and waited for with a COUNTED
  // vmcnt at the top of step s+2, so they have two MFMA runs to land.
  issue_step(0, 0);
  if (nsteps > 1) issue_step(1, 1);
  int rbuf = 0;   // ring buffer of this step; step+2 goes to the one before

  for (int step = 0; step < nsteps; ++step) {
    // this wave's loads of `step` have landed (all but the newest step's)
    if (step + 1 < nsteps)
      wait_vm<NX + NY>();
    else
      wait_vm<0>();
    // ... and everyone's; every wave is also done reading step-1's buffer,
    // which the loads issued below overwrite
    __builtin_amdgcn_s_barrier();

    const uint32_t boffs = (uint32_t)(rbuf * STAGE);
    i16x4 xlo[KS][MI], xhi[KS][MI], ylo[KS][NI], yhi[KS][NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      xlo[0][mi] = lds_read_tr16_b64<0>(aoff[mi][0] + boffs);
      xhi[0][mi] = lds_read_tr16_b64<0>(aoff[mi][1] + boffs);
    }
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      ylo[0][ni] = lds_read_tr16_b64<0>(boff[ni][0] + boffs);
      yhi[0][ni] = lds_read_tr16_b64<0>(boff[ni][1] + boffs);
    }
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      xlo[1][mi] = lds_read_tr16_b64<32 * BM * 2>(aoff[mi][0] + boffs);
      xhi[1][mi] = lds_read_tr16_b64<32 * BM * 2>(aoff[mi][1] + boffs);
    }
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      ylo[1][ni] = lds_read_tr16_b64<32 * BN * 2>(boff[ni][0] + boffs);
      yhi[1][ni] = lds_read_tr16_b64<32 * BN * 2>(boff[ni][1] + boffs);
    }

    if (step + 2 < nsteps) issue_step(step + 2, ring3_prev(rbuf));
    rbuf = ring3_next(rbuf);

    // raise issue priority for the MFMA run: co-resident waves still in
    // their address math yield issue slots to it
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      // LDS returns in order: k-block 0 is complete once at most the
      // k-block 1 reads are outstanding (the counter saturates at 15)
      wait_lgkm(ks == 0 ? (RD1 < 15 ? RD1 : 15) : 0);
      // the asm reads are invisible to the compiler's own wait insertion:
      // tie every fragment register to a point after the wait above
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
        frag_ready(xlo[ks][mi], xhi[ks][mi]);
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
        frag_ready(ylo[ks][ni], yhi[ks][ni]);
      __builtin_amdgcn_sched_barrier(0);
      bf16x8 xa[MI], yb[NI];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
        xa[mi] = __builtin_shufflevector(xlo[ks][mi], xhi[ks][mi], 0, 1, 2,
                                         3, 4, 5, 6, 7);
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
        yb[ni] = __builtin_shufflevector(ylo[ks][ni], yhi[ks][ni], 0, 1, 2,
                                         3, 4, 5, 6, 7);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              xa[mi], yb[ni], acc[mi][ni], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
  }

  // per-chunk partial, plain stores in channels-last element order; summed
  // by wgrad_reduce_kernel in fixed order
  const int ty = t / g.KW, tx = t % g.KW;
  float* dwc = dw + (int64_t)chunk * g.Cout * g.Cin * taps;
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ci = ci0 + (wr * MI + mi) * 16 + (lane >> 4) * 4 + r;
      if (ci >= g.Cin) continue;
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const int co = co0 + (wc * NI + ni) * 16 + (lane & 15);
        if (co >= g.Cout) continue;
        dwc[(((int64_t)co * g.KH + ty) * g.KW + tx) * g.Cin + ci] =
            acc[mi][ni][r];
      }
    }
  }
}

}  // namespace

// Block tile 64 ci x 128 co. 128x64 and 128x128 were measured too and never
// won a shape of the step (profiles/wgrad_tr.md); the kernel keeps BM, BN
// as template parameters, the geometry header and its host walk take both.
constexpr int WTR_BM = 64, WTR_BN = 128;

void wgrad_tr_launch(const WtrGeo& g, int nchunks, const bf16* x,
                     const bf16* dy, const bf16* zpage, float* dwp,
                     hipStream_t s) {
  const dim3 grid((unsigned)(cdiv(g.Cin, WTR_BM) * cdiv(g.Cout, WTR_BN) *
                             g.KH * g.KW * nchunks));
  // The XCD cell remap pays once the chunks are long enough for the L2 to
  // matter (measured: +4 us at 32^2, even at 64^2, -6..-37 % from 128^2
  // up).
  const int remap = g.M >= 65536;
  // 3 ring buffers = 72 KB
  const int lds = WTR_NBUF * WTR_KB * (WTR_BM + WTR_BN) * 2;
  lds_opt_in<&wgrad_tr_kernel<WTR_BM, WTR_BN>>(lds, "wgrad_tr");
  hipLaunchKernelGGL((wgrad_tr_kernel<WTR_BM, WTR_BN>), grid, dim3(256), lds,
                     s, x, dy, zpage, dwp, g, remap);
}

torch::Tensor lds_tr16_selftest() {
  auto out = torch::empty({4, 64, 8}, torch::dtype(torch::kInt16)
                                          .device(torch::kCUDA));
  hipLaunchKernelGGL(lds_tr16_selftest_kernel, dim3(1), dim3(64), 0,
                     at::cuda::getCurrentCUDAStream(),
                     out.data_ptr<int16_t>());
  HIP_CHECK_LAST();
  return out;
}

}  // namespace rthd
