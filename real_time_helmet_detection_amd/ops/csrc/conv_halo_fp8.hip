// Halo-tile fp8 (e4m3) conv for 3x3, stride 1, pad 1, Cin 128: the fp8 twin
// of conv_halo.hip.
//
// conv_fwd_fp8r_kernel stages one tap x 128 channels of input per K-step:
// over the 9 taps a block loads the same (8+2) x (16+2) pixel neighbourhood
// nine times. Here a workgroup owns an 8 x 16 tile of output pixels of one
// image, loads that tile's input ONCE with its one-pixel halo and keeps the
// [patch_px][128 B] image resident in LDS for all 9 taps; the A fragment of
// tap (dy, dx) is the same pair of ds_read_b128 at the patch pixel shifted
// by (dy, dx). Only the weights are loaded per K-step, 16 KB from the
// unchanged pack_weights_fp8 image [tap][Coutp][128] through a 3-deep ring.
//
// - One K-step = one tap = one mfma_scale_f32_16x16x128_f8f6f4 K block with
//   unit E8M0 scales. The taps run in the order of conv_fwd_fp8r_kernel and
//   lane l holds the same 32 channels (chunks 2*(l>>4), 2*(l>>4)+1, lo then
//   hi) of the same pixel / weight row, so every output element has the
//   same MFMA chain: results are bitwise equal to the 128x128 kernel.
// - Patch fill: global_load_lds, 16 B per lane, 23 1-KiB pieces dealt to
//   the 4 waves; pixels outside the image source the zero page. Patch and
//   weight stage are XOR-swizzled on the SOURCE chunk (conv_halo_fp8_geo.h)
//   so that every fragment read is 1-way.
// - Main loop: raw s_barrier with a counted vmcnt that leaves one K-step of
//   weights in flight; the fragment reads are inline asm with the kernel's
//   own lgkmcnt waits, as in conv_halo.hip.
// - 4 waves as 2 (tile-row halves) x 2 (64 output channels); fragment mi of
//   a wave is image row wr*MI + mi of the tile.
// The LDS layout, piece -> source maps, fragment offsets and wait counts
// live in conv_halo_fp8_geo.h and are walked on the host by
// tests/test_geo_checks.py; prologue, scalar and no-skip wide epilogue and
// launcher are conv_halo_common.h's.
#include <atomic>

#include "conv_halo_common.h"
#include "conv_halo_fp8_geo.h"

namespace rthd {

namespace {

DEV_INLINE i32x8 join(i32x4 lo, i32x4 hi) {
  return i32x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
}

// CIN: input channels (128 = the packed Cinp; one K block per tap). MI:
// image rows per wave; the tile is 2*MI rows x 16 px. WIDE: the output tile
// goes through LDS and leaves as 16-B stores (with a skip input: as fp32,
// the skip added on the way out).
// conv_halo_fp8_kernel reads its fragments with lds_read_b128 and waits of
// its own: the audit rule of lds_async.h applies to every edit.
template <int CIN, int MI, bool HAS_SKIP, bool WIDE, typename OUT_T>
__global__ __launch_bounds__(256)
void conv_halo_fp8_kernel(const fp8e4* __restrict__ x,
                          const fp8e4* __restrict__ wpk,
                          const float* __restrict__ scale,
                          const float* __restrict__ shift,
                          const fp8e4* __restrict__ skip,
                          const fp8e4* __restrict__ zpage,
                          OUT_T* __restrict__ y, HaloGeo g, int act) {
  static_assert(CIN == HALO_FP8_CIN, "one 128-channel K block per tap");
  static_assert(MI <= 4, "lgkmcnt counts 2*(MI-1) reads behind a wait");
  constexpr int TH = 2 * MI;
  using G = HaloFp8;
  constexpr int PATCH_BYTES = halo_patch_pieces<G>(TH) * 1024;
  constexpr int NSTEPS = 9;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ring = smem + PATCH_BYTES;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;

  int nblk, b, ty0, tx0;
  halo_cell_decompose(g, TH, blockIdx.x, &nblk, &b, &ty0, &tx0);
  halo_patch_fill<G, TH>(x, zpage, g, smem, wid, lane, b, ty0, tx0);

  // ---- weight ring: 128 rows x 128 B per K-step, 4 pieces per wave; piece
  // j is 32 rows (4 KiB of the packed image) below piece j - 1
  int wrow, wchunk;
  halo_fp8_wpiece_slot(0, wid, lane, &wrow, &wchunk);
  const fp8e4* wp0 = wpk + ((int64_t)nblk * HALO_BN + wrow) * CIN +
                     wchunk * G::EPC;
  const int64_t wtap = (int64_t)g.Coutp * CIN;
  auto issue_w = [&](int t, int buf) {
    const fp8e4* src = wp0 + t * wtap;
    char* base = ring + buf * G::WSTAGE + wid * 1024;
#pragma unroll
    for (int j = 0; j < G::WPIECES; ++j)
      __builtin_amdgcn_global_load_lds((glb_void*)(src + j * 32 * CIN),
          (lds_void*)(base + j * 4096), 16, 0, 0);
  };
  issue_w(0, 0);
  issue_w(1, 1);

  const uint32_t lds0 = lds_base(smem);
  // B fragment ni of this lane: row wc*64 + 16 ni + (lane & 15); the
  // swizzle term repeats every 16 rows, so ni is a 2-KiB immediate
  const uint32_t bbase0 = lds0 + PATCH_BYTES + halo_fp8_wfrag_off(wc, 0, lane);
  const uint32_t bbase1 = lds0 + PATCH_BYTES + halo_fp8_wfrag_off(wc, 1, lane);

  f32x4 acc[MI][4] = {};
  int rbuf = 0;  // ring buffer of this step; step+2 goes to the one before

#pragma unroll 1
  for (int t = 0; t < NSTEPS; ++t) {
    const int dy = t / 3, dx = t - 3 * dy;
    uint32_t alo[MI], ahi[MI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      alo[mi] = lds0 + halo_fp8_frag_off(wr * MI + mi, dy, dx, 0, lane);
      ahi[mi] = lds0 + halo_fp8_frag_off(wr * MI + mi, dy, dx, 1, lane);
    }

    // this wave's pieces of the step have landed: the patch and all
    // weights but the newest step's (halo_wait_count)
    if (t == NSTEPS - 1)
      wait_vm<0>();
    else
      wait_vm<G::WPIECES>();
    // ... and everyone's; every wave is also done reading the previous
    // step's ring buffer, which the loads issued below overwrite
    __builtin_amdgcn_s_barrier();

    const uint32_t bb0 = bbase0 + rbuf * G::WSTAGE;
    const uint32_t bb1 = bbase1 + rbuf * G::WSTAGE;
    i32x4 blo[4], bhi[4], flo[MI], fhi[MI];
    blo[0] = lds_read_b128<0, i32x4>(bb0);
    bhi[0] = lds_read_b128<0, i32x4>(bb1);
    blo[1] = lds_read_b128<2048, i32x4>(bb0);
    bhi[1] = lds_read_b128<2048, i32x4>(bb1);
    blo[2] = lds_read_b128<4096, i32x4>(bb0);
    bhi[2] = lds_read_b128<4096, i32x4>(bb1);
    blo[3] = lds_read_b128<6144, i32x4>(bb0);
    bhi[3] = lds_read_b128<6144, i32x4>(bb1);
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      flo[mi] = lds_read_b128<0, i32x4>(alo[mi]);
      fhi[mi] = lds_read_b128<0, i32x4>(ahi[mi]);
    }

    if (t + 2 < NSTEPS) issue_w(t + 2, ring3_prev(rbuf));
    rbuf = ring3_next(rbuf);

    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    i32x8 bfrag[4];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      // LDS returns in order: the B fragments and A rows 0..mi are
      // complete once at most the later A reads (two each) are outstanding
      wait_lgkm(2 * (MI - 1 - mi));
      // the asm reads are invisible to the compiler's own wait insertion:
      // tie the fragment registers to a point after the wait
      if (mi == 0) {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          frag_ready(blo[ni], bhi[ni]);
          bfrag[ni] = join(blo[ni], bhi[ni]);
        }
      }
      frag_ready(flo[mi], fhi[mi]);
      const i32x8 afrag = join(flo[mi], fhi[mi]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        acc[mi][ni] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            afrag, bfrag[ni], acc[mi][ni], 0, 0, 0, 0x7F7F7F7F, 0,
            0x7F7F7F7F);
      __builtin_amdgcn_sched_barrier(0);
    }
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
  }

  // ---- epilogue (conv_halo_common.h): the wide forms need whole 16-B
  // chunks of Cout
  const int col0 = halo_col0(nblk, wc, lane);
  float esc[4], esh[4];
  halo_load_scale_shift(scale, shift, col0, g.Cout, esc, esh);
  if (WIDE && HAS_SKIP) {
    // acc*scale + shift of the tile as fp32 [TH*16 px][128 ch] through LDS
    // (512-B rows; the 64-B group a 16-lane group writes is XORed by the
    // group's pixel quad so the four groups of a store hit different
    // banks); then each lane takes EPC channels of one pixel, adds one
    // vector load of the e4m3 skip, and stores 16 B. Same operations per
    // element as the scalar form below.
    constexpr int EPC = 16 / (int)sizeof(OUT_T);  // channels per lane
    constexpr int CPR = HALO_BN / EPC;            // lanes per tile row
    using skipv = __attribute__((ext_vector_type(EPC / 4))) int;
    __syncthreads();  // every wave is done with the patch and the ring
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int pl = (wr * MI + mi) * 16 + (lane >> 4) * 4 + r;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          const int grp = (wc * 4 + ni) ^ ((pl >> 2) & 3);
          float v = acc[mi][ni][r];
          v = v * esc[ni] + esh[ni];
          *reinterpret_cast<float*>(smem + pl * 512 + grp * 64 +
                                    (lane & 15) * 4) = v;
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < TH * 16 * CPR / 256; ++i) {
      const int idx = i * 256 + tid;
      const int pl = idx / CPR, ch = idx % CPR;
      const int c = nblk * HALO_BN + ch * EPC;
      if (c >= g.Cout) continue;
      const int cl = ch * EPC;
      const char* row = smem + pl * 512 +
                        (((cl >> 4) ^ ((pl >> 2) & 3)) << 6) + (cl & 15) * 4;
      const int64_t m =
          ((int64_t)b * g.H + ty0 + (pl >> 4)) * g.W + tx0 + (pl & 15);
      const skipv sv = *reinterpret_cast<const skipv*>(skip + m * g.Cout + c);
      i32x4 out;
#pragma unroll
      for (int q = 0; q < EPC / 4; ++q) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(row + q * 16);
        OUT_T o4[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const fp8e4 s8{(unsigned char)(((unsigned)sv[q] >> (8 * e)) & 0xff)};
          float v = a[e];
          v += ldf(&s8);
          v = apply_act(v, act);
          stf(&o4[e], v);
        }
        if constexpr (sizeof(OUT_T) == 1) {
          out[q] = (int)((unsigned)o4[0].v | ((unsigned)o4[1].v << 8) |
                         ((unsigned)o4[2].v << 16) | ((unsigned)o4[3].v << 24));
        } else {
          const unsigned short* h =
              reinterpret_cast<const unsigned short*>(o4);
          out[2 * q] = (int)((unsigned)h[0] | ((unsigned)h[1] << 16));
          out[2 * q + 1] = (int)((unsigned)h[2] | ((unsigned)h[3] << 16));
        }
      }
      *reinterpret_cast<i32x4*>(y + m * g.Cout + c) = out;
    }
  } else if (WIDE) {
    halo_epilogue_wide<MI>(acc, esc, esh, y, g, smem, nblk, b, ty0, tx0, tid,
                           wr, wc, act);
  } else {
    halo_epilogue_scalar<HAS_SKIP, MI>(acc, esc, esh, skip, y, g, b, ty0, tx0,
                                       wr, lane, col0, act);
  }
}

// 8 rows x 16 px: 23 KB of patch, 71 KB of LDS with the 3 x 16 KB ring,
// 2 blocks per CU (profiles/conv_fp8_halo.md)
constexpr int HALO_FP8_MI = 4;
constexpr int HALO_FP8_TH = 2 * HALO_FP8_MI;

std::atomic<int64_t> g_fp8_halo_launches{0};

template <int CIN, int MI, bool HAS_SKIP, bool WIDE, typename OUT_T>
void halo_fp8_launch_inst(const HaloGeo& hg, const ConvOperands& o, int act) {
  static_assert(!WIDE || halo_lds_bytes<HaloFp8>(2 * MI) >=
                             2 * MI * 16 * HALO_BN *
                                 (HAS_SKIP ? 4 : (int)sizeof(OUT_T)),
                "the output tile must fit in the LDS of the main loop");
  halo_launch<&conv_halo_fp8_kernel<CIN, MI, HAS_SKIP, WIDE, OUT_T>, HaloFp8,
              MI, fp8e4, OUT_T>("conv_halo_fp8", hg, o, act);
}

// The wide epilogues need whole 16-B chunks of output channels (16 e4m3 or
// 8 bf16); the other calls take the scalar one.
template <typename OUT_T>
void halo_fp8_launch_out(const HaloGeo& hg, const ConvOperands& o, int act) {
  constexpr int EPC = 16 / (int)sizeof(OUT_T);
  const bool wide = hg.Cout % EPC == 0;
  if (o.skip.defined()) {
    if (wide)
      halo_fp8_launch_inst<128, HALO_FP8_MI, true, true, OUT_T>(hg, o, act);
    else
      halo_fp8_launch_inst<128, HALO_FP8_MI, true, false, OUT_T>(hg, o, act);
  } else if (wide) {
    halo_fp8_launch_inst<128, HALO_FP8_MI, false, true, OUT_T>(hg, o, act);
  } else {
    halo_fp8_launch_inst<128, HALO_FP8_MI, false, false, OUT_T>(hg, o, act);
  }
}

}  // namespace

bool fp8_halo_eligible(const ConvGeo& g) {
  return halo_eligible(g, g.Cin == HALO_FP8_CIN, HALO_FP8_TH);
}

void launch_halo_fp8(const ConvGeo& g, const ConvOperands& o, int act,
                     bool out_fp8) {
  halo_check_eligible("conv_halo_fp8", g, fp8_halo_eligible(g), "128",
                      HALO_FP8_TH);
  const HaloGeo hg = make_halo_geo(g, HALO_FP8_TH);
  if (out_fp8) halo_fp8_launch_out<fp8e4>(hg, o, act);
  else         halo_fp8_launch_out<bf16>(hg, o, act);
  HIP_CHECK_LAST();
  g_fp8_halo_launches.fetch_add(1, std::memory_order_relaxed);
}

int64_t fp8_halo_launch_count() {
  return g_fp8_halo_launches.load(std::memory_order_relaxed);
}

}  // namespace rthd
