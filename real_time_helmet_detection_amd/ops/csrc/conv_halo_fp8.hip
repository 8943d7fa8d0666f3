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
// tests/test_conv_halo_fp8_geo.py.
#include <atomic>
#include <mutex>

#include "conv_common.h"
#include "conv_halo_fp8_geo.h"

namespace rthd {

namespace {

typedef __attribute__((address_space(3))) char lds_char;
using i32x4 = __attribute__((ext_vector_type(4))) int;

// One ds_read_b128 of the main loop, as inline asm (see conv_halo.hip and
// wgrad_tr.hip for the full argument). The compiler takes the "=v" result
// as written when the asm ends, while the data lands only at the kernel's
// lgkmcnt wait: between a read and its wait it must emit nothing that
// touches the result. AUDIT ON EVERY EDIT: in the .s of
// conv_halo_fp8_kernel the lines from the first ds_read_b128 of a K-step to
// its last s_waitcnt lgkmcnt hold only the reads, address arithmetic on
// OTHER registers, global_load_lds and MFMAs on already-waited fragments;
// ScratchSize is 0.
template <int OFF>
DEV_INLINE i32x4 lds_read16(uint32_t addr) {
  i32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2"
               : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}

// wait until at most n LDS reads are outstanding (n is 0, 2, 4 or 6 here)
DEV_INLINE void wait_lgkm(int n) {
  switch (n) {
    case 0: asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt lgkmcnt(2)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt lgkmcnt(6)" ::: "memory"); break;
    default: asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); break;
  }
}

DEV_INLINE i32x8 join(i32x4 lo, i32x4 hi) {
  return i32x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
}

// CIN: input channels (128 = the packed Cinp; one K block per tap). MI:
// image rows per wave; the tile is 2*MI rows x 16 px. WIDE: the output tile
// goes through LDS and leaves as 16-B stores (with a skip input: as fp32,
// the skip added on the way out).
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
  constexpr int NPIECE = ((TH + 2) * HALO_PW * HALO_FP8_RB + 1023) / 1024;
  constexpr int PATCH_BYTES = NPIECE * 1024;
  constexpr int NSTEPS = 9;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ring = smem + PATCH_BYTES;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;

  int nblk, b, ty0, tx0;
  halo_cell_decompose(g, TH, blockIdx.x, &nblk, &b, &ty0, &tx0);

  // ---- patch fill: piece f = 4i + wid, in pixel order
#pragma unroll
  for (int i = 0; i < (NPIECE + 3) / 4; ++i) {
    const int f = i * 4 + wid;
    if (f < NPIECE) {
      int p, c;
      halo_fp8_piece_slot(f, lane, &p, &c);
      const int64_t off = halo_fp8_src(g, TH, b, ty0, tx0, p, c);
      const fp8e4* src = off < 0 ? zpage : x + off;
      __builtin_amdgcn_global_load_lds((glb_void*)src,
          (lds_void*)(smem + f * 1024), 16, 0, 0);
    }
  }

  // ---- weight ring: 128 rows x 128 B per K-step, 4 pieces per wave; piece
  // j is 32 rows (4 KiB of the packed image) below piece j - 1
  int wrow, wchunk;
  halo_fp8_wpiece_slot(0, wid, lane, &wrow, &wchunk);
  const fp8e4* wp0 = wpk + ((int64_t)nblk * HALO_BN + wrow) * CIN +
                     wchunk * HALO_FP8_EPC;
  const int64_t wtap = (int64_t)g.Coutp * CIN;
  auto issue_w = [&](int t, int buf) {
    const fp8e4* src = wp0 + t * wtap;
    char* base = ring + buf * HALO_FP8_WSTAGE + wid * 1024;
#pragma unroll
    for (int j = 0; j < HALO_FP8_WPIECES; ++j)
      __builtin_amdgcn_global_load_lds((glb_void*)(src + j * 32 * CIN),
          (lds_void*)(base + j * 4096), 16, 0, 0);
  };
  issue_w(0, 0);
  issue_w(1, 1);

  const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_char*)smem;
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
    // weights but the newest step's (halo_fp8_wait_count)
    if (t == NSTEPS - 1)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(HALO_FP8_WPIECES) : "memory");
    // ... and everyone's; every wave is also done reading the previous
    // step's ring buffer, which the loads issued below overwrite
    __builtin_amdgcn_s_barrier();

    const uint32_t bb0 = bbase0 + rbuf * HALO_FP8_WSTAGE;
    const uint32_t bb1 = bbase1 + rbuf * HALO_FP8_WSTAGE;
    i32x4 blo[4], bhi[4], flo[MI], fhi[MI];
    blo[0] = lds_read16<0>(bb0);
    bhi[0] = lds_read16<0>(bb1);
    blo[1] = lds_read16<2048>(bb0);
    bhi[1] = lds_read16<2048>(bb1);
    blo[2] = lds_read16<4096>(bb0);
    bhi[2] = lds_read16<4096>(bb1);
    blo[3] = lds_read16<6144>(bb0);
    bhi[3] = lds_read16<6144>(bb1);
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      flo[mi] = lds_read16<0>(alo[mi]);
      fhi[mi] = lds_read16<0>(ahi[mi]);
    }

    const int wbuf = rbuf == 0 ? 2 : rbuf - 1;
    if (t + 2 < NSTEPS) issue_w(t + 2, wbuf);
    rbuf = rbuf == 2 ? 0 : rbuf + 1;

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
          asm volatile("" : "+v"(blo[ni]));
          asm volatile("" : "+v"(bhi[ni]));
          bfrag[ni] = join(blo[ni], bhi[ni]);
        }
      }
      asm volatile("" : "+v"(flo[mi]));
      asm volatile("" : "+v"(fhi[mi]));
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

  // ---- epilogue: y = act(acc*scale[c] + shift[c] (+skip)), the arithmetic
  // of conv_epilogue. acc[mi][ni][r] is image row ty0 + wr*MI + mi, pixel
  // tx0 + 4*(lane>>4) + r, channel col0 + 16 ni.
  const int col0 = nblk * HALO_BN + wc * 64 + (lane & 15);
  float esc[4], esh[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int c = col0 + ni * 16;
    esc[ni] = c < g.Cout ? scale[c] : 0.f;
    esh[ni] = c < g.Cout ? shift[c] : 0.f;
  }
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
    // the output tile [TH*16 px][128 ch] through LDS (rows of 128 elements;
    // the 16-B chunk index is XORed by the writing lane group's pixel quad
    // so the four groups of a store hit different banks), then 16 B per lane
    constexpr int ES = (int)sizeof(OUT_T);
    constexpr int EPC = 16 / ES;          // elements per 16-B chunk
    constexpr int CPR = HALO_BN / EPC;    // chunks per tile row
    constexpr int ROWB = HALO_BN * ES;
    __syncthreads();  // every wave is done with the patch and the ring
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int pl = (wr * MI + mi) * 16 + (lane >> 4) * 4 + r;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          const int cl = wc * 64 + ni * 16 + (lane & 15);
          float v = acc[mi][ni][r];
          v = v * esc[ni] + esh[ni];
          v = apply_act(v, act);
          const int chunk = (cl / EPC) ^ (((pl >> 2) & 3) << 1);
          stf(reinterpret_cast<OUT_T*>(smem + pl * ROWB + chunk * 16 +
                                       (cl % EPC) * ES), v);
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
      const int chunk = ch ^ (((pl >> 2) & 3) << 1);
      const i32x4 v =
          *reinterpret_cast<const i32x4*>(smem + pl * ROWB + chunk * 16);
      const int64_t m =
          ((int64_t)b * g.H + ty0 + (pl >> 4)) * g.W + tx0 + (pl & 15);
      *reinterpret_cast<i32x4*>(y + m * g.Cout + c) = v;
    }
  } else {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      const int64_t mrow =
          ((int64_t)b * g.H + ty0 + wr * MI + mi) * g.W + tx0 +
          (lane >> 4) * 4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t m = mrow + r;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          const int c = col0 + ni * 16;
          if (c >= g.Cout) continue;
          float v = acc[mi][ni][r];
          v = v * esc[ni] + esh[ni];
          if (HAS_SKIP) v += ldf(&skip[m * g.Cout + c]);
          v = apply_act(v, act);
          stf(&y[m * g.Cout + c], v);
        }
      }
    }
  }
}

// 8 rows x 16 px: 23 KB of patch, 71 KB of LDS with the 3 x 16 KB ring,
// 2 blocks per CU (profiles/conv_fp8_halo.md)
constexpr int HALO_FP8_MI = 4;
constexpr int HALO_FP8_TH = 2 * HALO_FP8_MI;

constexpr int halo_fp8_lds_bytes(int MI) {
  return ((2 * MI + 2) * HALO_PW * HALO_FP8_RB + 1023) / 1024 * 1024 +
         HALO_FP8_NBUF * HALO_FP8_WSTAGE;
}

std::atomic<int64_t> g_fp8_halo_launches{0};

template <int CIN, int MI, bool HAS_SKIP, bool WIDE, typename OUT_T>
void halo_fp8_launch_inst(const HaloGeo& hg, const ConvOperands& o, int act) {
  constexpr int lds = halo_fp8_lds_bytes(MI);
  static_assert(!WIDE || lds >= 2 * MI * 16 * HALO_BN *
                                    (HAS_SKIP ? 4 : (int)sizeof(OUT_T)),
                "the output tile must fit in the LDS of the main loop");
  auto* kern = &conv_halo_fp8_kernel<CIN, MI, HAS_SKIP, WIDE, OUT_T>;
  if (lds > 65536) {
    // above the 64 KB a kernel gets without opting in; once per device
    static std::mutex mu;
    static uint64_t done = 0;
    int dev = 0;
    TORCH_CHECK(hipGetDevice(&dev) == hipSuccess && dev < 64,
                "conv_halo_fp8: bad device");
    std::lock_guard<std::mutex> lk(mu);
    if (!((done >> dev) & 1)) {
      const hipError_t e = hipFuncSetAttribute(
          reinterpret_cast<const void*>(kern),
          hipFuncAttributeMaxDynamicSharedMemorySize, lds);
      TORCH_CHECK(e == hipSuccess, "conv_halo_fp8: cannot opt in to ", lds,
                  " B of LDS: ", hipGetErrorString(e));
      done |= (uint64_t)1 << dev;
    }
  }
  const dim3 grid((unsigned)(hg.B * hg.tiles_y * hg.tiles_x *
                             (hg.Coutp / HALO_BN)));
  hipLaunchKernelGGL(kern, grid, dim3(256), lds,
      at::cuda::getCurrentCUDAStream(), conv_ptr<const fp8e4>(o.x),
      conv_ptr<const fp8e4>(o.wpk), o.scale.data_ptr<float>(),
      o.shift.data_ptr<float>(), conv_ptr<const fp8e4>(o.skip),
      reinterpret_cast<const fp8e4*>(zero_page_bf16(o.x)),
      conv_ptr<OUT_T>(o.y), hg, act);
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
  return g.KH == 3 && g.KW == 3 && g.stride == 1 && g.pad == 1 &&
         g.Cin == HALO_FP8_CIN && g.Cinp == g.Cin &&
         g.H % HALO_FP8_TH == 0 && g.W % HALO_TW == 0;
}

void launch_halo_fp8(const ConvGeo& g, const ConvOperands& o, int act,
                     bool out_fp8) {
  TORCH_CHECK(fp8_halo_eligible(g), "conv_halo_fp8: needs 3x3 stride 1 pad "
              "1, Cin 128, H % ", HALO_FP8_TH, " == 0 and W % ", HALO_TW,
              " == 0; got k", g.KH, "x", g.KW, " s", g.stride, " p", g.pad,
              " Cin ", g.Cin, " H ", g.H, " W ", g.W);
  HaloGeo hg;
  hg.B = g.B; hg.H = g.H; hg.W = g.W; hg.Cin = g.Cin;
  hg.Cout = g.Cout; hg.Coutp = g.Coutp;
  hg.tiles_y = g.H / HALO_FP8_TH;
  hg.tiles_x = g.W / HALO_TW;
  if (out_fp8) halo_fp8_launch_out<fp8e4>(hg, o, act);
  else         halo_fp8_launch_out<bf16>(hg, o, act);
  HIP_CHECK_LAST();
  g_fp8_halo_launches.fetch_add(1, std::memory_order_relaxed);
}

int64_t fp8_halo_launch_count() {
  return g_fp8_halo_launches.load(std::memory_order_relaxed);
}

}  // namespace rthd
