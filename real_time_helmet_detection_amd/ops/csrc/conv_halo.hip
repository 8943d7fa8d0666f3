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
// conv_halo_geo.h and are walked on the host by tests/test_geo_checks.py;
// prologue, epilogues and launcher are conv_halo_common.h's.
#include "conv_halo_common.h"

namespace rthd {

namespace {

// CIN: input channels (64 or 128, = the packed Cinp). MI: image rows per
// wave; the tile is 2*MI rows x 16 px. WIDE (no skip): the bf16 tile goes
// through LDS and leaves as 16-B stores. STATS (WIDE only): the block also
// writes its row of the BN column partials sp1/sp2[tile][ld]
// (halo_epilogue_wide).
// conv_halo_kernel reads its fragments with lds_read_b128 and waits of its
// own: the audit rule of lds_async.h applies to every edit.
template <int CIN, int MI, bool HAS_SKIP, bool WIDE, bool STATS = false>
__global__ __launch_bounds__(256)
void conv_halo_kernel(const bf16* __restrict__ x,
                      const bf16* __restrict__ wpk,
                      const float* __restrict__ scale,
                      const float* __restrict__ shift,
                      const bf16* __restrict__ skip,
                      const bf16* __restrict__ zpage,
                      bf16* __restrict__ y, HaloGeo g, int act,
                      float* __restrict__ sp1, float* __restrict__ sp2,
                      int ld) {
  static_assert(!(HAS_SKIP && WIDE), "the wide epilogue has no skip input");
  static_assert(!STATS || WIDE, "stats ride on the wide epilogue");
  constexpr int TH = 2 * MI;
  using G = HaloBf16<CIN>;
  constexpr int KC = CIN / 32;
  constexpr int PATCH_BYTES = halo_patch_pieces<G>(TH) * 1024;
  constexpr int NSTEPS = 9 * KC;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ring = smem + PATCH_BYTES;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  int nblk, b, ty0, tx0;
  halo_cell_decompose(g, TH, blockIdx.x, &nblk, &b, &ty0, &tx0);
  halo_patch_fill<G, TH>(x, zpage, g, smem, wid, lane, b, ty0, tx0);

  // ---- weight ring: the K-step tile of conv.hip (128 rows x 64 B,
  // lds_off_row64), 2 pieces per wave
  const int st_row = tid >> 2;
  const int k8s = (tid & 3) ^ ((st_row >> 2) & 3);
  const bf16* wp0 = wpk + ((int64_t)nblk * HALO_BN + st_row) * CIN + k8s * 8;
  const bf16* wp1 = wp0 + 64 * CIN;
  const int64_t wtap = (int64_t)g.Coutp * CIN;
  auto issue_w = [&](int t, int kb, int buf) {
    const int64_t o = t * wtap + kb * 32;
    char* base = ring + buf * G::WSTAGE + wid * 1024;
    __builtin_amdgcn_global_load_lds((glb_void*)(wp0 + o), (lds_void*)base,
                                     16, 0, 0);
    __builtin_amdgcn_global_load_lds((glb_void*)(wp1 + o),
                                     (lds_void*)(base + 4096), 16, 0, 0);
  };
  issue_w(0, 0, 0);
  issue_w(1 / KC, 1 % KC, 1);

  const uint32_t lds0 = lds_base(smem);
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
      aoff[mi] = halo_frag_off<G>(wr * MI + mi, dy, dx, 0, lane);

#pragma unroll
    for (int kb = 0; kb < KC; ++kb) {
      // this wave's pieces of the step have landed: the patch and all
      // weights but the newest step's (halo_wait_count)
      if (t == 8 && kb == KC - 1)
        wait_vm<0>();
      else
        wait_vm<G::WPIECES>();
      // ... and everyone's; every wave is also done reading the previous
      // step's ring buffer, which the loads issued below overwrite
      __builtin_amdgcn_s_barrier();

      const uint32_t bb = bbase + rbuf * G::WSTAGE;
      bf16x8 bfrag[4], afrag[MI];
      bfrag[0] = lds_read_b128<0, bf16x8>(bb);
      bfrag[1] = lds_read_b128<1024, bf16x8>(bb);
      bfrag[2] = lds_read_b128<2048, bf16x8>(bb);
      bfrag[3] = lds_read_b128<3072, bf16x8>(bb);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
        afrag[mi] =
            lds_read_b128<0, bf16x8>(lds0 + (aoff[mi] ^ (kb << 6)));

      if (t * KC + kb + 2 < NSTEPS)
        issue_w(t + (kb + 2) / KC, (kb + 2) % KC, ring3_prev(rbuf));
      rbuf = ring3_next(rbuf);

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
          for (int ni = 0; ni < 4; ++ni) frag_ready(bfrag[ni]);
        }
        frag_ready(afrag[mi]);
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

  // ---- epilogue: wide (no skip, whole 16-B chunks of Cout) or scalar
  const int col0 = halo_col0(nblk, wc, lane);
  float esc[4], esh[4];
  halo_load_scale_shift(scale, shift, col0, g.Cout, esc, esh);
  if (WIDE)
    halo_epilogue_wide<MI, STATS>(acc, esc, esh, y, g, smem, nblk, b, ty0,
                                  tx0, tid, wr, wc, act, sp1, sp2, ld);
  else
    halo_epilogue_scalar<HAS_SKIP, MI>(acc, esc, esh, skip, y, g, b, ty0, tx0,
                                       wr, lane, col0, act);
}

// The tile is 8 rows x 16 px: 45 KB of patch at Cin 128, 69 KB of LDS with
// the ring, 2 blocks per CU. 16 x 16 (MI = 8: 81 KB patch, 1 block per CU,
// wave tile 128 px x 64 ch) loads less per pixel and measured 1.3-1.7x
// slower on every shape (profiles/conv_halo.md); the kernel keeps MI as a
// template parameter, the geometry header and its host walk take both.
constexpr int HALO_MI = 4;
constexpr int HALO_TH = 2 * HALO_MI;

// sp: the stats instantiation's partial rows (sp.p1 == nullptr: none)
struct HaloStatsOut {
  float* p1 = nullptr;
  float* p2 = nullptr;
  int ld = 0;
};

template <int CIN, int MI, bool HAS_SKIP, bool WIDE, bool STATS = false>
void halo_launch_inst(const HaloGeo& hg, const ConvOperands& o, int act,
                      const HaloStatsOut& sp = HaloStatsOut{}) {
  static_assert(!WIDE || halo_lds_bytes<HaloBf16<CIN>>(2 * MI) >=
                             2 * MI * 16 * 256,
                "the output tile must fit in the LDS of the main loop");
  halo_launch<&conv_halo_kernel<CIN, MI, HAS_SKIP, WIDE, STATS>,
              HaloBf16<CIN>, MI, bf16, bf16>("conv_halo", hg, o, act, sp.p1,
                                             sp.p2, sp.ld);
}

// The wide epilogue needs whole 16-B chunks of output channels and has no
// skip input; the other calls take the scalar one. Stats ride on the wide
// epilogue only (halo_stats_ok).
template <int CIN>
void halo_launch_cin(const HaloGeo& hg, const ConvOperands& o, int act,
                     const HaloStatsOut& sp) {
  if (sp.p1)
    halo_launch_inst<CIN, HALO_MI, false, true, true>(hg, o, act, sp);
  else if (o.skip.defined())
    halo_launch_inst<CIN, HALO_MI, true, false>(hg, o, act);
  else if (hg.Cout % 8 == 0)
    halo_launch_inst<CIN, HALO_MI, false, true>(hg, o, act);
  else
    halo_launch_inst<CIN, HALO_MI, false, false>(hg, o, act);
}

void launch_halo_impl(const ConvGeo& g, const ConvOperands& o, int act,
                      const HaloStatsOut& sp) {
  halo_check_eligible("conv_halo", g, halo_eligible(g), "64 or 128", HALO_TH);
  const HaloGeo hg = make_halo_geo(g, HALO_TH);
  if (g.Cin == 128) halo_launch_cin<128>(hg, o, act, sp);
  else              halo_launch_cin<64>(hg, o, act, sp);
  HIP_CHECK_LAST();
}

}  // namespace

bool halo_eligible(const ConvGeo& g) {
  return halo_eligible(g, g.Cin == 64 || g.Cin == 128, HALO_TH);
}

void launch_halo(const ConvGeo& g, const ConvOperands& o, int act) {
  launch_halo_impl(g, o, act, HaloStatsOut{});
}

bool halo_stats_ok(const ConvGeo& g) {
  return halo_eligible(g) && g.Cout % 8 == 0;
}

int64_t halo_stats_rows(const ConvGeo& g) {
  return (int64_t)g.B * (g.H / HALO_TH) * (g.W / HALO_TW);
}

void launch_halo_stats(const ConvGeo& g, const ConvOperands& o, int act,
                       float* p1, float* p2, int ld) {
  TORCH_CHECK(halo_stats_ok(g) && !o.skip.defined(),
              "conv_halo stats: needs an eligible shape, Cout % 8 == 0 and "
              "no skip");
  TORCH_CHECK(p1 && p2 && ld >= g.Cout && ld % 4 == 0,
              "conv_halo stats: bad partial rows");
  launch_halo_impl(g, o, act, HaloStatsOut{p1, p2, ld});
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

// The halo variant with its stats epilogue, forced (tests, kbench). p1/p2:
// optional caller-owned fp32 [rows >= tiles][cols >= Cout] partial buffers
// (unit column stride, 16-B aligned rows); rows [0, tiles) x columns
// [0, Cout) are written and nothing else. Returns {y, p1, p2}.
std::vector<torch::Tensor> conv_fwd_halo_stats(
    torch::Tensor x, torch::Tensor wpk, torch::Tensor scale,
    torch::Tensor shift, int64_t KH, int64_t KW, int64_t stride, int64_t pad,
    int64_t Cout, int64_t act, c10::optional<torch::Tensor> p1,
    c10::optional<torch::Tensor> p2) {
  TORCH_CHECK(wpk.scalar_type() == at::kBFloat16,
              "conv_fwd_halo_stats: bf16 packed weights required");
  TORCH_CHECK(p1.has_value() == p2.has_value(),
              "conv_fwd_halo_stats: p1 and p2 go together");
  const ConvGeo g = make_conv_geo("conv_fwd_halo_stats", x, wpk, KH, KW,
                                  stride, pad, Cout, 64);
  auto o = prep_conv_operands(g, x, wpk, scale, shift, c10::nullopt,
                              at::kBFloat16, at::kBFloat16);
  TORCH_CHECK(halo_stats_ok(g), "conv_fwd_halo_stats: shape not eligible");
  const int64_t rows = halo_stats_rows(g);
  torch::Tensor a, b;
  if (p1.has_value()) {
    a = *p1;
    b = *p2;
    for (const torch::Tensor* t : {&a, &b})
      TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat &&
                  t->dim() == 2 && t->size(0) >= rows && t->size(1) >= Cout &&
                  t->stride(1) == 1 && t->stride(0) == a.stride(0) &&
                  t->stride(0) % 4 == 0 &&
                  reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0,
                  "conv_fwd_halo_stats: bad partial buffer");
  } else {
    a = torch::empty({rows, Cout}, o.x.options().dtype(at::kFloat));
    b = torch::empty_like(a);
  }
  launch_halo_stats(g, o, (int)act, a.data_ptr<float>(), b.data_ptr<float>(),
                    (int)a.stride(0));
  return {o.y, a, b};
}

}  // namespace rthd
