// Geometry of the transposed-read bf16 wgrad (wgrad_tr.hip): the LDS image,
// the lane maps of the staging and fragment-read instructions, and the
// source-pixel map. Plain C++ with no HIP or torch dependency, so the same
// functions the kernel calls are walked lane by lane on the host
// (tests/wgrad_tr_geo_check.cpp) before anything runs on a GPU.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define WTR_HD __host__ __device__ inline
#else
#define WTR_HD inline
#endif

namespace rthd {

// px rows per K-step (one LDS stage): two 16x16x32 MFMA k-blocks
constexpr int WTR_KB = 64;

struct WtrGeo {
  int B, H, W, Cin, Ho, Wo, Cout;
  int KH, KW, stride, pad;
  int M;
  int chunk_len;
};

// Pixel-chunk length of one block, shared by both bf16 wgrad kernels (and
// by the host walk): about 1024 blocks at the register-transpose kernel's
// 64x64 tiles, rounded up to 128 px. 1x1 convs have no tap reuse to keep
// in L2 and prefer longer K runs per block: the chunk-size sweep measured
// 2048 fastest (65 us vs 82 at the formula's 1024 for 128ch @128^2).
// forced >= 128 (RTHD_WGRAD_CHUNK) overrides, rounded up to 128.
WTR_HD int wtr_chunk_len(int M, int Cin, int Cout, int taps, int forced) {
  const int tiles = ((Cin + 63) / 64) * ((Cout + 63) / 64) * taps;
  const int nchunks = 1024 / tiles > 1 ? 1024 / tiles : 1;
  int len = ((M + nchunks - 1) / nchunks + 127) / 128 * 128;
  if (taps == 1 && M >= 4096 && len < 2048) len = 2048;
  if (forced >= 128) len = (forced + 127) / 128 * 128;
  return len;
}

// ------------------------------ block -> cell -------------------------------
// Blocks are dealt round-robin over the XCDs (block b and b + NUM_XCD share
// one). The cells that share data are numbered consecutively, so with
// cell = block id they land on all XCDs and every XCD's L2 streams all of
// the data. The remap gives the blocks of XCD k a contiguous range of cells
// instead (the first G % NUM_XCD XCDs take one cell more): a permutation of
// 0 .. G - 1 for any grid size G. Speed only.
constexpr int NUM_XCD = 8;

WTR_HD int xcd_cell_remap(int cell, int G) {
  const int k = cell % NUM_XCD, j = cell / NUM_XCD, rem = G % NUM_XCD;
  return k * (G / NUM_XCD) + (k < rem ? k : rem) + j;
}

// ------------------------------ LDS image -----------------------------------
// One operand tile is [WTR_KB px][CH ch] bf16 in MEMORY order (channels
// contiguous), CH = 64 or 128, i.e. 128-B or 256-B rows of 16-B chunks.
// The chunk index is XOR-swizzled by the row so that the transposed read
// of a 16x16x32 operand (per 32-lane half: two 4-row x 32-B blocks 8 rows
// apart) touches all 64 banks once:
//   256-B rows: the row term vanishes mod 64 banks, so all 16 chunk values
//     of the 8 rows x 2 chunks must differ: swz = (row&3)<<2 | (row>>2)&3.
//   128-B rows: row parity picks the bank half; the 4 rows of one parity
//     (bit 1 of the row, and the 8-row group) spread over chunk bits 2, 1.
WTR_HD int wtr_swz(int row, int CH) {
  return CH == 128 ? (((row & 3) << 2) | ((row >> 2) & 3))
                   : ((((row >> 1) & 1) << 2) | (((row >> 3) & 1) << 1));
}

// byte offset of 16-B channel chunk `chunk` of px row `row`: the store image
// and the read address both go through this one function
WTR_HD int wtr_lds_off(int row, int chunk, int CH) {
  return row * (CH * 2) + ((chunk ^ wtr_swz(row, CH)) << 4);
}

// Staging: wave-instruction f (0 .. WTR_KB*CH/512 - 1) writes the 1024
// lane-linear bytes [f*1024, f*1024 + 1024) of the tile, 16 B per lane.
// Returns the px row and the SOURCE channel chunk whose data must land
// there for the image to equal wtr_lds_off's layout.
WTR_HD int wtr_stage_byte(int f, int lane) { return f * 1024 + lane * 16; }

WTR_HD void wtr_stage_slot(int f, int lane, int CH, int* row, int* chunk) {
  const int byte = wtr_stage_byte(f, lane);
  const int r = byte / (CH * 2);
  const int pc = (byte % (CH * 2)) >> 4;
  *row = r;
  *chunk = pc ^ wtr_swz(r, CH);
}

// Transposed fragment read (ds_read_b64_tr_b16): byte address lane `lane`
// supplies for 16-channel block `frag`, MFMA k-block `ks` (32 px) and
// half `h` (k-slots j = 4h .. 4h+3). Lane 4q+p of 16-lane group g names px
// row 32ks + 8g + 4h + q, channels 16frag + 4p .. +3; lane i of the group
// receives channel 16frag + i of those 4 rows.
WTR_HD int wtr_tr_addr(int frag, int ks, int h, int lane, int CH) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int row = 32 * ks + 8 * g + 4 * h + q;
  return wtr_lds_off(row, 2 * frag + (p >> 1), CH) + 8 * (p & 1);
}

// ---------------------------- source-pixel map ------------------------------
// output pixel m = (b*Ho + oy)*Wo + ox, kept incrementally per staged row
struct WtrPix { int b, oy, ox; };

WTR_HD void wtr_pix_init(int m, int Ho, int Wo, WtrPix* p) {
  p->b = m / (Ho * Wo);
  const int r = m - p->b * (Ho * Wo);
  p->oy = r / Wo;
  p->ox = r - p->oy * Wo;
}

// advance by n pixels given db = n / (Ho*Wo), dq = n % (Ho*Wo) / Wo,
// dr = n % Wo: branch-free, one carry per level (dq < Ho and dr < Wo)
WTR_HD void wtr_pix_advance(WtrPix* p, int db, int dq, int dr, int Ho,
                            int Wo) {
  int ox = p->ox + dr;
  const int cx = ox >= Wo;
  ox -= cx ? Wo : 0;
  int oy = p->oy + dq + cx;
  const int cy = oy >= Ho;
  oy -= cy ? Ho : 0;
  p->ox = ox;
  p->oy = oy;
  p->b += db + cy;
}

// element offset into x (NHWC) of channel c at the input pixel that tap
// (dyt, dxt) pairs with output pixel m, or -1 = the zero page: halo,
// pixels past the chunk end, channels at or above Cin
WTR_HD int64_t wtr_x_src(const WtrGeo& g, const WtrPix& p, int m, int px_end,
                         int dyt, int dxt, int c) {
  const int iy = p.oy * g.stride + dyt;
  const int ix = p.ox * g.stride + dxt;
  // bitwise &, and the offset computed either way: no branch in the stager
  const bool ok = (m < px_end) & (iy >= 0) & (iy < g.H) & (ix >= 0) &
                  (ix < g.W) & (c < g.Cin);
  const int64_t off = (int64_t)((p.b * g.H + iy) * g.W + ix) * g.Cin + c;
  return ok ? off : -1;
}

// element offset into dy (NHWC), or -1 = the zero page
WTR_HD int64_t wtr_dy_src(const WtrGeo& g, int m, int px_end, int c) {
  const bool ok = (m < px_end) & (c < g.Cout);
  return ok ? (int64_t)m * g.Cout + c : -1;
}

}  // namespace rthd
