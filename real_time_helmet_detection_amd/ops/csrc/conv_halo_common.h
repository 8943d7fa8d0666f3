// The skeleton the halo-tile 3x3 convs share (conv_halo.hip,
// conv_halo_fp8.hip): the patch fill of the prologue, the scale/shift load,
// the scalar and the no-skip wide epilogue, and on the host the HaloGeo
// fill, the eligibility rule with its refusal message and the launcher.
// Each kernel file keeps its main loop (weight-ring issue, fragment reads,
// MFMA), its tile constants, its instantiation choice and its entry points;
// G is the dtype's geometry traits (conv_halo_geo.h).
//
// The device helpers take the block's identity as plain ints: 4 waves as 2
// (tile-row halves, wr) x 2 (64 output channels, wc); n block nblk of the
// tile whose first output pixel is (b, ty0, tx0), from halo_cell_decompose.
// (Carried in a struct, the compiler pairs ty0 and tx0 into vector
// arithmetic and the kernels' register counts move; the epilogues' pointer
// arguments that are __restrict__ in the kernels are __restrict__ here for
// the same reason: profiles/lds_async_refactor.md.)
#pragma once

#include "conv_halo_geo.h"
#include "lds_async.h"

namespace rthd {

// ------------------------------ device side ---------------------------------

// Prologue, after halo_cell_decompose: issue the patch fill, piece
// f = 4i + wid in pixel order, 16 B per lane; pixels outside the image
// source the zero page.
template <typename G, int TH, typename T>
DEV_INLINE void halo_patch_fill(const T* x, const T* zpage, const HaloGeo& g,
                                char* smem, int wid, int lane, int b, int ty0,
                                int tx0) {
  constexpr int NPIECE = halo_patch_pieces<G>(TH);
#pragma unroll
  for (int i = 0; i < (NPIECE + 3) / 4; ++i) {
    const int f = i * 4 + wid;
    if (f < NPIECE) {
      int p, c;
      halo_piece_slot<G>(f, lane, &p, &c);
      const int64_t off = halo_src<G>(g, TH, b, ty0, tx0, p, c);
      const T* src = off < 0 ? zpage : x + off;
      __builtin_amdgcn_global_load_lds((glb_void*)src,
          (lds_void*)(smem + f * 1024), 16, 0, 0);
    }
  }
}

// Epilogue: y = act(acc*scale[c] + shift[c] (+skip)), the arithmetic of
// conv_epilogue. acc[mi][ni][r] is image row ty0 + wr*MI + mi, pixel
// tx0 + 4*(lane>>4) + r, channel halo_col0 + 16 ni.
DEV_INLINE int halo_col0(int nblk, int wc, int lane) {
  return nblk * HALO_BN + wc * 64 + (lane & 15);
}

DEV_INLINE void halo_load_scale_shift(const float* __restrict__ scale,
                                      const float* __restrict__ shift,
                                      int col0, int Cout, float (&esc)[4],
                                      float (&esh)[4]) {
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    const int c = col0 + ni * 16;
    esc[ni] = c < Cout ? scale[c] : 0.f;
    esh[ni] = c < Cout ? shift[c] : 0.f;
  }
}

// one store per element; any Cout
template <bool HAS_SKIP, int MI, typename SKIP_T, typename OUT_T>
DEV_INLINE void halo_epilogue_scalar(const f32x4 (&acc)[MI][4],
                                     const float (&esc)[4],
                                     const float (&esh)[4],
                                     const SKIP_T* __restrict__ skip,
                                     OUT_T* __restrict__ y, const HaloGeo& g,
                                     int b, int ty0, int tx0, int wr,
                                     int lane, int col0, int act) {
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

// No skip, Cout in whole 16-B chunks: the output tile [TH*16 px][128 ch]
// goes through LDS (rows of 128 elements; the 16-B chunk index is XORed by
// the writing lane group's pixel quad so the four groups of a store hit
// different banks) and leaves as 16 B per lane. The tile must fit in the
// LDS of the main loop (the caller's static_assert).
//
// STATS (bf16 out, TH = 8): the block also writes row `tile` of the BN
// column partials sp1/sp2[tile][ld] = sum / sum of squares of the ROUNDED
// outputs of its 128 pixels, channels nblk*128 .. < Cout. In the store loop
// a thread keeps one channel octet (256 % CPR == 0) and adds its 8 pixels
// from the registers it stores from; the 16 pixel groups of a channel are
// then summed through the tile's LDS in group order by wave 0 and leave as
// 16-B stores. Every partial row has one owner: no atomics, no memset,
// fixed order.
template <int MI, bool STATS = false, typename OUT_T>
DEV_INLINE void halo_epilogue_wide(const f32x4 (&acc)[MI][4],
                                   const float (&esc)[4],
                                   const float (&esh)[4],
                                   OUT_T* __restrict__ y, const HaloGeo& g,
                                   char* smem,
                                   int nblk, int b, int ty0, int tx0,
                                   int tid, int wr, int wc, int act,
                                   float* __restrict__ sp1 = nullptr,
                                   float* __restrict__ sp2 = nullptr,
                                   int ld = 0) {
  const int lane = tid & 63;
  constexpr int TH = 2 * MI;
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
  if constexpr (STATS) {
    static_assert(ES == 2 && 256 % CPR == 0, "bf16 tile, fixed octet");
    constexpr int NG = 256 / CPR;  // pixel groups; thread = (group, octet)
    const int ch = tid % CPR, pg = tid / CPR;
    const int c = nblk * HALO_BN + ch * EPC;
    float s[8] = {}, q[8] = {};
    if (c < g.Cout) {
#pragma unroll
      for (int i = 0; i < TH * 16 / NG; ++i) {
        const int pl = i * NG + pg;
        const int chunk = ch ^ (((pl >> 2) & 3) << 1);
        const i32x4 v =
            *reinterpret_cast<const i32x4*>(smem + pl * ROWB + chunk * 16);
        const int64_t m =
            ((int64_t)b * g.H + ty0 + (pl >> 4)) * g.W + tx0 + (pl & 15);
        *reinterpret_cast<i32x4*>(y + m * g.Cout + c) = v;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t u = (uint32_t)v[k];
          const float lo = __uint_as_float(u << 16);
          const float hi = __uint_as_float(u & 0xffff0000u);
          s[2 * k] += lo;
          q[2 * k] += lo * lo;
          s[2 * k + 1] += hi;
          q[2 * k + 1] += hi * hi;
        }
      }
    }
    __syncthreads();  // every thread has read its part of the tile
    // red[sum | sumsq][group][128 channels], 2 * NG * 512 B <= the tile
    static_assert(2 * NG * HALO_BN * 4 <= TH * 16 * ROWB, "partials fit");
    float* red = reinterpret_cast<float*>(smem);
    f32x4* r1 = reinterpret_cast<f32x4*>(red + pg * HALO_BN + ch * EPC);
    f32x4* r2 = reinterpret_cast<f32x4*>(red + (NG + pg) * HALO_BN + ch * EPC);
    r1[0] = f32x4{s[0], s[1], s[2], s[3]};
    r1[1] = f32x4{s[4], s[5], s[6], s[7]};
    r2[0] = f32x4{q[0], q[1], q[2], q[3]};
    r2[1] = f32x4{q[4], q[5], q[6], q[7]};
    __syncthreads();
    if (tid < 64) {
      const int which = tid >> 5, c4 = (tid & 31) * 4;
      const float* src = red + which * NG * HALO_BN + c4;
      f32x4 a = *reinterpret_cast<const f32x4*>(src);
#pragma unroll
      for (int k = 1; k < NG; ++k)
        a += *reinterpret_cast<const f32x4*>(src + k * HALO_BN);
      const int cg = nblk * HALO_BN + c4;
      const int64_t tile = ((int64_t)b * g.tiles_y + ty0 / TH) * g.tiles_x +
                           tx0 / HALO_TW;
      if (cg < g.Cout)
        *reinterpret_cast<f32x4*>((which ? sp2 : sp1) + tile * ld + cg) = a;
    }
    return;
  }
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
}

// ------------------------------- host side ----------------------------------

// shapes a halo kernel with TH x 16 tiles takes; cin_ok is the kernel's
// own rule on the input channels
inline bool halo_eligible(const ConvGeo& g, bool cin_ok, int TH) {
  return g.KH == 3 && g.KW == 3 && g.stride == 1 && g.pad == 1 && cin_ok &&
         g.Cinp == g.Cin && g.H % TH == 0 && g.W % HALO_TW == 0;
}

// the refusal of a shape that is not eligible; cin_rule as in "Cin 64 or 128"
inline void halo_check_eligible(const char* who, const ConvGeo& g, bool ok,
                                const char* cin_rule, int TH) {
  TORCH_CHECK(ok, who, ": needs 3x3 stride 1 pad 1, Cin ", cin_rule,
              ", H % ", TH, " == 0 and W % ", HALO_TW, " == 0; got k", g.KH,
              "x", g.KW, " s", g.stride, " p", g.pad, " Cin ", g.Cin, " H ",
              g.H, " W ", g.W);
}

inline HaloGeo make_halo_geo(const ConvGeo& g, int TH) {
  HaloGeo hg;
  hg.B = g.B; hg.H = g.H; hg.W = g.W; hg.Cin = g.Cin;
  hg.Cout = g.Cout; hg.Coutp = g.Coutp;
  hg.tiles_y = g.H / TH;
  hg.tiles_x = g.W / HALO_TW;
  return hg;
}

// one block per (tile, n block); LDS = patch + weight ring, opted in to
// where that is above 64 KB. The zero page is 16 zero bytes for any T.
// KERN(const T* x, wpk, scale, shift, skip, zpage, OUT_T* y, HaloGeo, act,
//      extra...)
template <auto KERN, typename G, int MI, typename T, typename OUT_T,
          typename... Extra>
void halo_launch(const char* who, const HaloGeo& hg, const ConvOperands& o,
                 int act, Extra... extra) {
  constexpr int lds = halo_lds_bytes<G>(2 * MI);
  lds_opt_in<KERN>(lds, who);
  const dim3 grid((unsigned)(hg.B * hg.tiles_y * hg.tiles_x *
                             (hg.Coutp / HALO_BN)));
  hipLaunchKernelGGL(KERN, grid, dim3(256), lds,
      at::cuda::getCurrentCUDAStream(), conv_ptr<const T>(o.x),
      conv_ptr<const T>(o.wpk), o.scale.data_ptr<float>(),
      o.shift.data_ptr<float>(), conv_ptr<const T>(o.skip),
      reinterpret_cast<const T*>(zero_page_bf16(o.x)), conv_ptr<OUT_T>(o.y),
      hg, act, extra...);
}

}  // namespace rthd
