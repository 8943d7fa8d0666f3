// Halo-tile bf16 conv for 3x3, stride 1, pad 1.
//
// conv.hip stages one tap x 32 channels of input per K-step: over the 9
// taps a block loads the same (8+2) x (16+2) pixel neighbourhood nine
// times, shifted by one pixel per tap. Here a workgroup owns a TH x 16
// tile of output pixels of one image, loads that tile's input ONCE with its
// one-pixel halo and keeps the [patch_px][Cin] image resident in LDS for the
// whole K loop; the A fragment of tap (dy, dx) is the same ds_read_b128 at
// the patch pixel shifted by (dy, dx). Only the weights are loaded per
// K-step, from the unchanged packed [tap][Coutp][Cinp] image through the
// 3-deep 8-KB ring of conv.hip.
//
// - K order (tap-major, 32-channel steps), MFMA and the lane -> (row,
//   channel chunk) map are those of conv_fwd_bf16_kernel, so every output
//   element has the same accumulation chain: results are bitwise equal to
//   the 128x128 variants.
// - Patch fill: global_load_lds, 16 B per lane, 1-KiB pieces dealt to the 4
//   waves; pixels outside the image source the zero page. The image is
//   XOR-swizzled on the SOURCE chunk (conv_halo_geo.h) so that a fragment
//   read is 1-way from any start pixel.
// - Main loop: raw s_barrier with a counted vmcnt that leaves one K-step of
//   weights in flight; the fragment reads are inline asm with the kernel's
//   own lgkmcnt waits (through the builtin the compiler drains vmcnt(0)
//   before every LDS read while a global_load_lds is pending).
// - 4 waves as 2 (tile rows) x 2 (64 output channels); fragment mi of a
//   wave is image row wr*MI + mi of the tile, so the epilogue maps
//   fragments to rows of the image and not to 16 consecutive m.
// The LDS layout, piece -> source map and fragment offsets live in
// conv_halo_geo.h and are walked on the host by tests/test_conv_halo_geo.py.
#include <mutex>

#include "conv_common.h"
#include "conv_halo_geo.h"

namespace rthd {

namespace {

typedef __attribute__((address_space(3))) char lds_char;

// One fragment read of the main loop, as inline asm (see wgrad_tr.hip for
// the full argument). The compiler takes the "=v" result as written when
// the asm ends, while the data lands only at the kernel's lgkmcnt wait:
// between a read and its wait it must emit nothing that touches the
// result. AUDIT ON EVERY EDIT: in the .s of conv_halo_kernel the lines
// from the first ds_read_b128 of a K-step to its last s_waitcnt lgkmcnt
// hold only the reads, address arithmetic on OTHER registers,
// global_load_lds and MFMAs on already-waited fragments; ScratchSize is 0.
template <int OFF>
DEV_INLINE bf16x8 lds_read16(uint32_t addr) {
  bf16x8 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2"
               : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}

// wait until at most n LDS reads are outstanding (n is 0..7 here)
DEV_INLINE void wait_lgkm(int n) {
  switch (n) {
    case 0: asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt lgkmcnt(1)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt lgkmcnt(2)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt lgkmcnt(3)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt lgkmcnt(5)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt lgkmcnt(6)" ::: "memory"); break;
    default: asm volatile("s_waitcnt lgkmcnt(7)" ::: "memory"); break;
  }
}

// CIN: input channels (64 or 128, = the packed Cinp). MI: image rows per
// wave; the tile is 2*MI rows x 16 px. WIDE (no skip): the bf16 tile goes
// through LDS and leaves as 16-B stores.
template <int CIN, int MI, bool HAS_SKIP, bool WIDE>
__global__ __launch_bounds__(256)
void conv_halo_kernel(const bf16* __restrict__ x,
                      const bf16* __restrict__ wpk,
                      const float* __restrict__ scale,
                      const float* __restrict__ shift,
                      const bf16* __restrict__ skip,
                      const bf16* __restrict__ zpage,
                      bf16* __restrict__ y, HaloGeo g, int act) {
  static_assert(!(HAS_SKIP && WIDE), "the wide epilogue has no skip input");
  constexpr int TH = 2 * MI;
  constexpr int RB = CIN * 2;
  constexpr int KC = CIN / 32;
  constexpr int NPIECE = ((TH + 2) * HALO_PW * RB + 1023) / 1024;
  constexpr int PATCH_BYTES = NPIECE * 1024;
  constexpr int NSTEPS = 9 * KC;
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
      halo_piece_slot(f, lane, RB, &p, &c);
      const int64_t off = halo_src(g, TH, b, ty0, tx0, p, c);
      const bf16* src = off < 0 ? zpage : x + off;
      __builtin_amdgcn_global_load_lds((glb_void*)src,
          (lds_void*)(smem + f * 1024), 16, 0, 0);
    }
  }

  // ---- weight ring: the K-step tile of conv.hip (128 rows x 64 B,
  // lds_off_row64), 2 pieces per wave
  const int st_row = tid >> 2;
  const int k8s = (tid & 3) ^ ((st_row >> 2) & 3);
  const bf16* wp0 = wpk + ((int64_t)nblk * HALO_BN + st_row) * CIN + k8s * 8;
  const bf16* wp1 = wp0 + 64 * CIN;
  const int64_t wtap = (int64_t)g.Coutp * CIN;
  auto issue_w = [&](int t, int kb, int buf) {
    const int64_t o = t * wtap + kb * 32;
    char* base = ring + buf * HALO_WSTAGE + wid * 1024;
    __builtin_amdgcn_global_load_lds((glb_void*)(wp0 + o), (lds_void*)base,
                                     16, 0, 0);
    __builtin_amdgcn_global_load_lds((glb_void*)(wp1 + o),
                                     (lds_void*)(base + 4096), 16, 0, 0);
  };
  issue_w(0, 0, 0);
  issue_w(1 / KC, 1 % KC, 1);

  const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_char*)smem;
  // B fragment ni of this lane: row wc*64 + 16 ni + (lane & 15); the
  // swizzle term repeats every 16 rows, so ni is a 1-KiB immediate
  const uint32_t bbase =
      lds0 + PATCH_BYTES + lds_off_row64(wc * 64 + (lane & 15), lane >> 4);

  f32x4 acc[MI][4] = {};
  int rbuf = 0;  // ring buffer of this step; step+2 goes to the one before

#pragma unroll 1
  for (int t = 0; t < 9; ++t) {
    const int dy = t / 3, dx = t - 3 * dy;
    uint32_t aoff[MI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
      aoff[mi] = halo_frag_off(wr * MI + mi, dy, dx, 0, lane, RB);

#pragma unroll
    for (int kb = 0; kb < KC; ++kb) {
      // this wave's pieces of the step have landed: the patch and all
      // weights but the newest step's (halo_wait_count)
      if (t == 8 && kb == KC - 1)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(HALO_WPIECES) : "memory");
      // ... and everyone's; every wave is also done reading the previous
      // step's ring buffer, which the loads issued below overwrite
      __builtin_amdgcn_s_barrier();

      const uint32_t bb = bbase + rbuf * HALO_WSTAGE;
      bf16x8 bfrag[4], afrag[MI];
      bfrag[0] = lds_read16<0>(bb);
      bfrag[1] = lds_read16<1024>(bb);
      bfrag[2] = lds_read16<2048>(bb);
      bfrag[3] = lds_read16<3072>(bb);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
        afrag[mi] = lds_read16<0>(lds0 + (aoff[mi] ^ (kb << 6)));

      const int wbuf = rbuf == 0 ? 2 : rbuf - 1;
      if (t * KC + kb + 2 < NSTEPS)
        issue_w(t + (kb + 2) / KC, (kb + 2) % KC, wbuf);
      rbuf = rbuf == 2 ? 0 : rbuf + 1;

      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        // LDS returns in order: the B fragments and A rows 0..mi are
        // complete once at most the later A reads are outstanding
        wait_lgkm(MI - 1 - mi);
        // the asm reads are invisible to the compiler's own wait
        // insertion: tie the fragment registers to a point after the wait
        if (mi == 0) {
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) asm volatile("" : "+v"(bfrag[ni]));
        }
        asm volatile("" : "+v"(afrag[mi]));
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              afrag[mi], bfrag[ni], acc[mi][ni], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
    }
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
  if (WIDE) {
    // the bf16 tile [TH*16 px][128 ch] through LDS (256-B rows; the 32-B
    // pair a 16-lane group writes is XORed by the group's pixel quad so
    // the four groups of a store hit different banks), then 16 B per lane
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
          const int chunk = (cl >> 3) ^ (((pl >> 2) & 3) << 1);
          stf(reinterpret_cast<bf16*>(smem + pl * 256 + chunk * 16 +
                                      (cl & 7) * 2), v);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < TH; ++i) {
      const int idx = i * 256 + tid;
      const int pl = idx >> 4, ch = idx & 15;
      const int c = nblk * HALO_BN + ch * 8;
      if (c >= g.Cout) continue;
      const int chunk = ch ^ (((pl >> 2) & 3) << 1);
      const bf16x8 v =
          *reinterpret_cast<const bf16x8*>(smem + pl * 256 + chunk * 16);
      const int64_t m =
          ((int64_t)b * g.H + ty0 + (pl >> 4)) * g.W + tx0 + (pl & 15);
      *reinterpret_cast<bf16x8*>(y + m * g.Cout + c) = v;
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

// The tile is 8 rows x 16 px: 45 KB of patch at Cin 128, 69 KB of LDS with
// the ring, 2 blocks per CU. 16 x 16 (MI = 8: 81 KB patch, 1 block per CU,
// wave tile 128 px x 64 ch) loads less per pixel and measured 1.3-1.7x
// slower on every shape (profiles/conv_halo.md); the kernel keeps MI as a
// template parameter, the geometry header and its host walk take both.
constexpr int HALO_MI = 4;
constexpr int HALO_TH = 2 * HALO_MI;

constexpr int halo_lds_bytes(int CIN, int MI) {
  return ((2 * MI + 2) * HALO_PW * CIN * 2 + 1023) / 1024 * 1024 +
         HALO_NBUF * HALO_WSTAGE;
}

template <int CIN, int MI, bool HAS_SKIP, bool WIDE>
void halo_launch_inst(const HaloGeo& hg, const ConvOperands& o, int act) {
  constexpr int lds = halo_lds_bytes(CIN, MI);
  static_assert(!WIDE || lds >= 2 * MI * 16 * 256,
                "the output tile must fit in the LDS of the main loop");
  auto* kern = &conv_halo_kernel<CIN, MI, HAS_SKIP, WIDE>;
  if (lds > 65536) {
    // above the 64 KB a kernel gets without opting in; once per device
    static std::mutex mu;
    static uint64_t done = 0;
    int dev = 0;
    TORCH_CHECK(hipGetDevice(&dev) == hipSuccess && dev < 64,
                "conv_halo: bad device");
    std::lock_guard<std::mutex> lk(mu);
    if (!((done >> dev) & 1)) {
      const hipError_t e = hipFuncSetAttribute(
          reinterpret_cast<const void*>(kern),
          hipFuncAttributeMaxDynamicSharedMemorySize, lds);
      TORCH_CHECK(e == hipSuccess, "conv_halo: cannot opt in to ", lds,
                  " B of LDS: ", hipGetErrorString(e));
      done |= (uint64_t)1 << dev;
    }
  }
  const dim3 grid((unsigned)(hg.B * hg.tiles_y * hg.tiles_x *
                             (hg.Coutp / HALO_BN)));
  hipLaunchKernelGGL(kern, grid, dim3(256), lds,
      at::cuda::getCurrentCUDAStream(), conv_ptr<const bf16>(o.x),
      conv_ptr<const bf16>(o.wpk), o.scale.data_ptr<float>(),
      o.shift.data_ptr<float>(), conv_ptr<const bf16>(o.skip),
      zero_page_bf16(o.x), conv_ptr<bf16>(o.y), hg, act);
}

// The wide epilogue needs whole 16-B chunks of output channels and has no
// skip input; the other calls take the scalar one.
template <int CIN>
void halo_launch_cin(const HaloGeo& hg, const ConvOperands& o, int act) {
  if (o.skip.defined())
    halo_launch_inst<CIN, HALO_MI, true, false>(hg, o, act);
  else if (hg.Cout % 8 == 0)
    halo_launch_inst<CIN, HALO_MI, false, true>(hg, o, act);
  else
    halo_launch_inst<CIN, HALO_MI, false, false>(hg, o, act);
}

}  // namespace

bool halo_eligible(const ConvGeo& g) {
  return g.KH == 3 && g.KW == 3 && g.stride == 1 && g.pad == 1 &&
         (g.Cin == 64 || g.Cin == 128) && g.Cinp == g.Cin &&
         g.H % HALO_TH == 0 && g.W % HALO_TW == 0;
}

void launch_halo(const ConvGeo& g, const ConvOperands& o, int act) {
  TORCH_CHECK(halo_eligible(g), "conv_halo: needs 3x3 stride 1 pad 1, Cin "
              "64 or 128, H % ", HALO_TH, " == 0 and W % ", HALO_TW,
              " == 0; got k", g.KH, "x", g.KW, " s", g.stride, " p", g.pad,
              " Cin ", g.Cin, " H ", g.H, " W ", g.W);
  HaloGeo hg;
  hg.B = g.B; hg.H = g.H; hg.W = g.W; hg.Cin = g.Cin;
  hg.Cout = g.Cout; hg.Coutp = g.Coutp;
  hg.tiles_y = g.H / HALO_TH;
  hg.tiles_x = g.W / HALO_TW;
  if (g.Cin == 128) halo_launch_cin<128>(hg, o, act);
  else              halo_launch_cin<64>(hg, o, act);
  HIP_CHECK_LAST();
}

torch::Tensor conv_fwd_halo(torch::Tensor x, torch::Tensor wpk,
                            torch::Tensor scale, torch::Tensor shift,
                            c10::optional<torch::Tensor> skip,
                            int64_t KH, int64_t KW, int64_t stride,
                            int64_t pad, int64_t Cout, int64_t act) {
  TORCH_CHECK(wpk.scalar_type() == at::kBFloat16,
              "conv_fwd_halo: bf16 packed weights required");
  const ConvGeo g = make_conv_geo("conv_fwd_halo", x, wpk, KH, KW, stride,
                                  pad, Cout, 64);
  auto o = prep_conv_operands(g, x, wpk, scale, shift, skip, at::kBFloat16,
                              at::kBFloat16);
  launch_halo(g, o, (int)act);
  return o.y;
}

}  // namespace rthd
