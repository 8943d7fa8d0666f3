// Tap-row bf16 wgrad: the three taps of one kernel row from one staged X.
//
// wgrad_tr.hip gives every tap a block of its own, so the nine taps of a
// 3x3 load the same dY chunk and the same X pixels (shifted) nine times; its
// loads run at the bandwidth ceiling while the MFMAs idle. For stride 1,
// pad 1 the taps dx = -1, 0, +1 of one kernel row read X at px - 1, px,
// px + 1 of the same [px][ch] image, so here a block owns a whole tap ROW:
// - X is staged once per 64-px K-step for the pixels p0 - 1 .. p0 + 64 at
//   input row oy + dyt (64 px plus a one-pixel apron each side, rounded up
//   to 1-KiB global_load_lds pieces); dY is staged once as in wgrad_tr.
// - The A fragment of tap dx is the same ds_read_b64_tr_b16 pair one LDS
//   row up or down; B fragments are read once for the three taps. Three
//   times the MFMAs per byte loaded and per source-map evaluation.
// - The shifted read wraps into the neighbouring image row at ox == 0
//   (tap -1) and ox == Wo - 1 (tap +1). With Wo % 32 == 0 that can only be
//   k-slot 0 or 31 of a k-block; that one 16-bit element is zeroed in the
//   register after the wait (wave-uniform per k-block). Not in LDS: the
//   image is shared by the three taps.
// - Chunks, k-slots, MFMA and partial layout are those of wgrad_tr.hip and
//   a masked element is the zero the zero page delivers there: at equal
//   chunk length the result is bitwise equal to variant 'tr'.
// - The ring (3 deep), the counted vmcnt, the raw barrier, the asm reads
//   with counted lgkmcnt and the setprio bracket are wgrad_tr's. Waves
//   issue different numbers of X pieces (9 pieces over 4 waves), so each
//   wave's vmcnt count is its own, picked by a wave-uniform branch.
// The geometry lives in wgrad_row_geo.h (on top of wgrad_tr_geo.h) and is
// walked on the host by tests/test_geo_checks.py. Resource usage of the kept
// instantiation is recorded in profiles/wgrad_row.md.
#include "lds_async.h"
#include "wgrad_row_geo.h"

namespace rthd {

namespace {

using u32x2 = __attribute__((ext_vector_type(2))) uint32_t;

constexpr int WROW_NBUF = 3;   // LDS ring depth

// zero the edge element of a fragment half: `word` is all ones in the
// lanes and k-blocks that hold no edge
template <int REG>
DEV_INLINE i16x4 row_mask(i16x4 v, uint32_t word) {
  u32x2 u = __builtin_bit_cast(u32x2, v);
  u[REG] &= word;
  return __builtin_bit_cast(i16x4, u);
}

// wgrad_row_kernel reads its fragments with lds_read_tr16_b64 and waits of
// its own: the audit rule of lds_async.h applies to every edit.
template <int BM, int BN>
__global__ __launch_bounds__(256, 2)
void wgrad_row_kernel(const bf16* __restrict__ x, const bf16* __restrict__ dy,
                      const bf16* __restrict__ zpage, float* __restrict__ dw,
                      WtrGeo g, int xcd_remap) {
  constexpr int MI = BM / 32, NI = BN / 32;   // 16-wide fragments per wave
  constexpr int NP = (WROW_USED * BM * 2 + 1023) / 1024;   // X pieces
  constexpr int XB = NP * 1024;               // bytes of the X image
  constexpr int YB = WTR_KB * BN * 2;
  constexpr int STAGE = XB + YB;
  constexpr int NXMAX = (NP + 3) / 4;         // X pieces of wave 0
  constexpr int NXMIN = NP / 4;               // ... of wave 3
  constexpr int NY = YB / 4096;
  constexpr int KS = WTR_KB / 32;             // MFMA k-blocks per step
  constexpr int RD1 = 2 * (3 * MI + NI);      // fragment reads per k-block
  static_assert(KS == 2, "the fragment reads below are written for KS = 2");
  static_assert(NXMAX - NXMIN <= 1, "two wait counts");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  // One block per (kernel row, px-chunk, ci-tile, co-tile) cell, chunk-
  // major, with xcd_cell_remap (wgrad_tr_geo.h): the rows x tiles blocks
  // that share a px chunk get consecutive cells, and one XCD takes a
  // contiguous cell range. Speed only.
  const int ci_t = (g.Cin + BM - 1) / BM, co_t = (g.Cout + BN - 1) / BN;
  int cell = blockIdx.x;
  if (xcd_remap) cell = xcd_cell_remap(cell, gridDim.x);
  const int z = cell / (ci_t * co_t);
  const int ty = z % 3;
  const int chunk = z / 3;
  const int ci0 = (cell % ci_t) * BM;
  const int co0 = (cell / ci_t % co_t) * BN;
  const int dyt = ty - 1;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid >> 1, wc = wid & 1;
  const int nxw = (NP - wid + 3) / 4;         // X pieces of this wave

  const int px_start = chunk * g.chunk_len;
  const int px_end = min(px_start + g.chunk_len, g.M);
  const int nsteps = (px_end - px_start + WTR_KB - 1) / WTR_KB;

  // staging slots of this lane: piece i of wave w is wave-instruction
  // f = 4i + w of the image (wtr_stage_slot)
  WtrPix pix[NXMAX];
  int xrow[NXMAX], xch[NXMAX], yrow[NY], ych[NY];
#pragma unroll
  for (int i = 0; i < NXMAX; ++i) {
    int c;
    wtr_stage_slot(i * 4 + wid, lane, BM, &xrow[i], &c);
    xch[i] = ci0 + c * 8;
    wrow_pix_init(px_start - WROW_APRON + xrow[i], g.Ho, g.Wo, &pix[i]);
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
    for (int i = 0; i < NXMAX; ++i) {
      if (i < NXMIN || i < nxw) {   // wave-uniform
        const int64_t off = wrow_x_src(g, pix[i], p0 - WROW_APRON + xrow[i],
                                       xrow[i], px_end, dyt, xch[i]);
        const bf16* src = off < 0 ? zpage : x + off;
        __builtin_amdgcn_global_load_lds((glb_void*)src,
            (lds_void*)(base + wtr_stage_byte(i * 4 + wid, lane)), 16, 0, 0);
        wtr_pix_advance(&pix[i], adv_b, adv_q, adv_r, g.Ho, g.Wo);
      }
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
  // rows further: an offset immediate; the swizzle has period 16 rows)
  const uint32_t lds0 = lds_base(smem);
  uint32_t aoff[3][MI][2], boff[NI][2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
        aoff[t][mi][h] =
            lds0 + wrow_tr_addr(wr * MI + mi, 0, h, t - 1, lane, BM);
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
      boff[ni][h] = lds0 + XB + wtr_tr_addr(wc * NI + ni, 0, h, lane, BN);
  }
  const uint32_t mword_lo = wrow_mask_word(-1, lane);
  const uint32_t mword_hi = wrow_mask_word(+1, lane);
  // ox of the step's first pixel (a multiple of 32 below Wo), walked per step
  int oxs = __builtin_amdgcn_readfirstlane(px_start % g.Wo);

  f32x4 acc[3][MI][NI] = {};

  issue_step(0, 0);
  if (nsteps > 1) issue_step(1, 1);
  int rbuf = 0;   // ring buffer of this step; step+2 goes to the one before

  for (int step = 0; step < nsteps; ++step) {
    // this wave's loads of `step` have landed (all but the newest step's)
    if (step + 1 < nsteps) {
      if (nxw == NXMAX)
        wait_vm<NXMAX + NY>();
      else
        wait_vm<NXMIN + NY>();
    } else {
      wait_vm<0>();
    }
    // ... and everyone's; every wave is also done reading step-1's buffer,
    // which the loads issued below overwrite
    __builtin_amdgcn_s_barrier();

    const uint32_t boffs = (uint32_t)(rbuf * STAGE);
    i16x4 xlo[KS][3][MI], xhi[KS][3][MI], ylo[KS][NI], yhi[KS][NI];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        xlo[0][t][mi] = lds_read_tr16_b64<0>(aoff[t][mi][0] + boffs);
        xhi[0][t][mi] = lds_read_tr16_b64<0>(aoff[t][mi][1] + boffs);
      }
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      ylo[0][ni] = lds_read_tr16_b64<0>(boff[ni][0] + boffs);
      yhi[0][ni] = lds_read_tr16_b64<0>(boff[ni][1] + boffs);
    }
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        xlo[1][t][mi] = lds_read_tr16_b64<32 * BM * 2>(aoff[t][mi][0] + boffs);
        xhi[1][t][mi] = lds_read_tr16_b64<32 * BM * 2>(aoff[t][mi][1] + boffs);
      }
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      ylo[1][ni] = lds_read_tr16_b64<32 * BN * 2>(boff[ni][0] + boffs);
      yhi[1][ni] = lds_read_tr16_b64<32 * BN * 2>(boff[ni][1] + boffs);
    }

    if (step + 2 < nsteps) issue_step(step + 2, ring3_prev(rbuf));
    rbuf = ring3_next(rbuf);

    // edge masks of the two k-blocks (wave-uniform selects)
    uint32_t mlo[KS], mhi[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      int oxk = oxs + 32 * ks;
      oxk -= oxk >= g.Wo ? g.Wo : 0;
      mlo[ks] = wrow_edge(-1, oxk, g.Wo) ? mword_lo : 0xffffffffu;
      mhi[ks] = wrow_edge(+1, oxk, g.Wo) ? mword_hi : 0xffffffffu;
    }
    oxs += adv_r;
    oxs -= oxs >= g.Wo ? g.Wo : 0;

    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      // LDS returns in order: k-block 0 is complete once at most 15 of the
      // RD1 >= 15 reads of k-block 1 are outstanding (the counter's range)
      static_assert(RD1 >= 15, "lgkmcnt(15) must cover k-block 0");
      wait_lgkm(ks == 0 ? 15 : 0);
      // the asm reads are invisible to the compiler's own wait insertion:
      // tie every fragment register to a point after the wait above
#pragma unroll
      for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
          frag_ready(xlo[ks][t][mi], xhi[ks][t][mi]);
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
        frag_ready(ylo[ks][ni], yhi[ks][ni]);
      __builtin_amdgcn_sched_barrier(0);
      bf16x8 yb[NI];
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
        yb[ni] = __builtin_shufflevector(ylo[ks][ni], yhi[ks][ni], 0, 1, 2,
                                         3, 4, 5, 6, 7);
#pragma unroll
      for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          i16x4 lo = xlo[ks][t][mi], hi = xhi[ks][t][mi];
          if (t == 0) lo = row_mask<0>(lo, mlo[ks]);
          if (t == 2) hi = row_mask<1>(hi, mhi[ks]);
          const bf16x8 xa =
              __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
          for (int ni = 0; ni < NI; ++ni)
            acc[t][mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                xa, yb[ni], acc[t][mi][ni], 0, 0, 0);
        }
      __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
  }

  // per-chunk partials of the three taps, plain stores in channels-last
  // element order [chunk][co][ty][tx][ci]; summed by wgrad_reduce_kernel
  float* dwc = dw + (int64_t)chunk * g.Cout * g.Cin * 9;
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
#pragma unroll
        for (int t = 0; t < 3; ++t)
          dwc[(((int64_t)co * 3 + ty) * 3 + t) * g.Cin + ci] =
              acc[t][mi][ni][r];
      }
    }
  }
}

// one tile's launch; BM, BN stay template parameters so that a sweep can
// instantiate another tile
template <int BM, int BN>
void row_launch_tile(const WtrGeo& g, int nchunks, const bf16* x,
                     const bf16* dy, const bf16* zpage, float* dwp,
                     hipStream_t s) {
  const dim3 grid((unsigned)(cdiv(g.Cin, BM) * cdiv(g.Cout, BN) * 3 *
                             nchunks));
  // The XCD cell remap was re-measured for this kernel: even at 32^2 and
  // 64^2 (+-2 us), -3 % at 128^2, -9 % at 256^2 (profiles/wgrad_row.md)
  const int remap = g.M >= 65536;
  // 3 ring buffers
  const int lds = WROW_NBUF * (wrow_x_pieces(BM) * 1024 + WTR_KB * BN * 2);
  lds_opt_in<&wgrad_row_kernel<BM, BN>>(lds, "wgrad_row");
  hipLaunchKernelGGL((wgrad_row_kernel<BM, BN>), grid, dim3(256), lds, s, x,
                     dy, zpage, dwp, g, remap);
}

}  // namespace

// Block tile 3 taps x 64 ci x 128 co. 3 x 64 x 64 was measured too: ahead
// only at 128ch @128^2 (121 vs 129 us) with a chunk target of its own, and
// behind on the two 256^2 shapes; 3 x 128 x 64 needs 96 accumulator plus
// 112 fragment registers and does not fit two waves per SIMD
// (profiles/wgrad_row.md).
constexpr int WROW_BM = 64, WROW_BN = 128;

void wgrad_row_launch(const WtrGeo& g, int nchunks, const bf16* x,
                      const bf16* dy, const bf16* zpage, float* dwp,
                      hipStream_t s) {
  TORCH_CHECK(wrow_eligible(g) && g.chunk_len % 128 == 0,
              "wgrad_row: ineligible shape");
  row_launch_tile<WROW_BM, WROW_BN>(g, nchunks, x, dy, zpage, dwp, s);
}

}  // namespace rthd
