// Geometry of the tap-row bf16 wgrad (wgrad_row.hip): one block computes the
// three taps of one kernel row of a 3x3 stride-1 pad-1 conv from ONE staged
// X image. On top of wgrad_tr_geo.h (LDS offsets, swizzle, staging lane
// map, dY source map) this header adds the apron rows of the X image, the
// shifted fragment reads, the per-pixel source map of a whole tap row, the
// image-row edge masks and the kernel's chunk rule. Plain C++: walked on the
// host by tests/wgrad_row_geo_check.cpp.
#pragma once

#include "wgrad_tr_geo.h"

namespace rthd {

// The X image of one K-step is [rows][CH] like the tr kernel's, for the
// pixels p0 - 1 .. p0 + 64 of the output-pixel order, all at input row
// oy + dyt: LDS row r holds pixel p0 - WROW_APRON + r. Tap dx reads its
// A fragments WROW_APRON + dx rows down. The 66 rows are rounded up to whole
// 1-KiB staging pieces; the rows past 65 are filled from the zero page.
constexpr int WROW_APRON = 1;
constexpr int WROW_USED = WTR_KB + 2;

WTR_HD int wrow_x_pieces(int CH) {
  return (WROW_USED * CH * 2 + 1023) / 1024;
}
WTR_HD int wrow_x_rows(int CH) { return wrow_x_pieces(CH) * 1024 / (CH * 2); }

// X staging pieces wave `wid` of 4 issues per K-step: pieces wid, wid + 4, ..
WTR_HD int wrow_x_wave_pieces(int wid, int CH) {
  return (wrow_x_pieces(CH) - wid + 3) / 4;
}

// Pixel-chunk length of one block of the row kernel: about `WROW_BLOCKS`
// blocks at its 64 ci x 128 co x 3-tap tiles, rounded up to 128 px so that
// (with Wo % 32 == 0) no 32-px k-block straddles an image row. 512 is one
// resident wave of blocks (256 CUs x 2 per CU): a second wave costs more in
// tail and fp32 partials than it gains (sweep in profiles/wgrad_row.md).
// forced >= 128 (RTHD_WGRAD_CHUNK) overrides, rounded up to 128.
constexpr int WROW_BLOCKS = 512;

WTR_HD int wrow_chunk_len(int M, int Cin, int Cout, int forced) {
  const int tiles = ((Cin + 63) / 64) * ((Cout + 127) / 128) * 3;
  const int nchunks = WROW_BLOCKS / tiles > 1 ? WROW_BLOCKS / tiles : 1;
  int len = ((M + nchunks - 1) / nchunks + 127) / 128 * 128;
  if (forced >= 128) len = (forced + 127) / 128 * 128;
  return len;
}

// Shapes the row kernel computes: 3x3, stride 1, pad 1 (so Ho = H, Wo = W),
// whole 32-px k-blocks per image row, 16-B channel groups.
WTR_HD bool wrow_eligible(const WtrGeo& g) {
  return g.KH == 3 && g.KW == 3 && g.stride == 1 && g.pad == 1 &&
         g.Ho == g.H && g.Wo == g.W && g.Wo % 32 == 0 && g.Cin % 8 == 0 &&
         g.Cout % 8 == 0;
}

// A-fragment read of tap dx (-1, 0, +1): wtr_tr_addr's lane map, the px row
// moved down by the apron and the shift. Through wtr_lds_off like the fill.
WTR_HD int wrow_tr_addr(int frag, int ks, int h, int dx, int lane, int CH) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int row = WROW_APRON + dx + 32 * ks + 8 * g + 4 * h + q;
  return wtr_lds_off(row, 2 * frag + (p >> 1), CH) + 8 * (p & 1);
}

// (b, oy, ox) of pixel m >= -1 by FLOOR division: pixel -1, the apron of
// the first chunk, is (-1, Ho - 1, Wo - 1), from which wtr_pix_advance walks
// on correctly.
WTR_HD void wrow_pix_init(int m, int Ho, int Wo, WtrPix* p) {
  if (m < 0) {
    p->b = -1;
    p->oy = Ho - 1;
    p->ox = Wo + m;
  } else {
    wtr_pix_init(m, Ho, Wo, p);
  }
}

// element offset into x (NHWC) of channel c of the pixel LDS row `row` of
// the step starting at p0 holds, i.e. output pixel m = p0 - WROW_APRON + row
// (pix = its decomposition) moved dyt image rows, or -1 = the zero page:
// rows above or below the image, pixels outside [0, M), pixels past the
// apron of the chunk end (dY is zero from px_end on, and the pixel px_end
// itself feeds tap +1 of px_end - 1), the filler rows, channels >= Cin.
WTR_HD int64_t wrow_x_src(const WtrGeo& g, const WtrPix& p, int m, int row,
                          int px_end, int dyt, int c) {
  const int iy = p.oy + dyt;
  const bool ok = (row < WROW_USED) & (m >= 0) & (m < g.M) & (m <= px_end) &
                  (iy >= 0) & (iy < g.H) & (c < g.Cin);
  const int64_t off = (int64_t)((p.b * g.H + iy) * g.W + p.ox) * g.Cin + c;
  return ok ? off : -1;
}

// ------------------------------ edge masks ----------------------------------
// The shifted read wraps into the neighbouring image row: tap -1 at ox == 0
// reads the previous row's last pixel, tap +1 at ox == Wo - 1 the next
// row's first. A 32-px k-block lies in one image row and starts at a
// multiple of 32, so only its k-slot 0 (tap -1) and k-slot 31 (tap +1) can
// be such a pixel. Slot (g, j) is element j & 3 of half j >> 2 in lane
// group g: slot 0 is the low 16 bits of register 0 of the low half in
// lanes 0-15, slot 31 the high 16 bits of register 1 of the high half in
// lanes 48-63. oxk = ox of the k-block's first pixel (wave-uniform).
WTR_HD bool wrow_edge(int dx, int oxk, int Wo) {
  return dx < 0 ? oxk == 0 : dx > 0 ? oxk + 32 == Wo : false;
}
WTR_HD int wrow_mask_half(int dx) { return dx > 0; }
WTR_HD int wrow_mask_reg(int dx) { return dx > 0; }
// AND mask for that register of tap dx in a k-block that holds the edge
WTR_HD uint32_t wrow_mask_word(int dx, int lane) {
  return dx < 0 ? (lane < 16 ? 0xffff0000u : 0xffffffffu)
       : dx > 0 ? (lane >= 48 ? 0x0000ffffu : 0xffffffffu)
                : 0xffffffffu;
}

}  // namespace rthd
