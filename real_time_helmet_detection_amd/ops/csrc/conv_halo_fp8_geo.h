// Geometry of the halo-tile 3x3 fp8 conv (conv_halo_fp8.hip): what differs
// from conv_halo_geo.h, which supplies the tile, the patch pixel numbering,
// the piece bytes and the block decomposition. Plain C++ with no HIP or
// torch dependency: the functions the kernel calls are walked lane by lane
// on the host (tests/conv_halo_fp8_geo_check.cpp).
//
// The patch is stored [p][128 B]: one e4m3 pixel of 128 channels per row,
// cut into eight 16-B chunks of 16 channels. One K-step is one tap and the
// whole row: the A fragment of tap (dy, dx) for tile row r is TWO
// ds_read_b128 per lane, lane l reading chunks 2*(l>>4) (lo) and
// 2*(l>>4) + 1 (hi) of pixel (r+dy)*18 + (l&15) + dx — the lane -> k map of
// conv_fwd_fp8r_kernel with the tap folded into the start pixel.
#pragma once

#include "conv_halo_geo.h"

namespace rthd {

constexpr int HALO_FP8_CIN = 128;      // channels = bytes per patch pixel
constexpr int HALO_FP8_RB = 128;       // patch row bytes
constexpr int HALO_FP8_EPC = 16;       // e4m3 elements per 16-B chunk
constexpr int HALO_FP8_WSTAGE = HALO_BN * 128;  // ring stage: 128 rows x 128 B
constexpr int HALO_FP8_NBUF = 3;       // weight ring depth
constexpr int HALO_FP8_WPIECES = 4;    // weight pieces per wave per K-step

HALO_HD int halo_fp8_patch_pieces(int TH) {
  return (halo_patch_px(TH) * HALO_FP8_RB + 1023) / 1024;
}

// XOR term on the 3-bit chunk index. One ds_read_b128 of a fragment half
// takes the chunks {h, 2+h, 4+h, 6+h} of 16 consecutive pixels from any
// start: halo_swz of the bf16 kernel is 2-way under that map, this one is
// 1-way (bit 2 of p picks chunk bit 0, bit 1 of p chunk bit 2; the host
// walk is the proof).
HALO_HD int halo_fp8_swz(int p) {
  return ((p >> 2) & 1) | (((p >> 1) & 1) << 2);
}

// byte offset of 16-B chunk `chunk` of patch pixel p: fill image and read
// address both go through this function
HALO_HD int halo_fp8_lds_off(int p, int chunk) {
  return p * HALO_FP8_RB + ((chunk ^ halo_fp8_swz(p)) << 4);
}

// Fill: piece f writes the lane-linear bytes [f*1024, f*1024 + 1024)
// (halo_piece_byte). Returns the patch pixel and the SOURCE chunk whose
// data must land at this lane's 16 B.
HALO_HD void halo_fp8_piece_slot(int f, int lane, int* p, int* chunk) {
  const int byte = halo_piece_byte(f, lane);
  const int q = byte / HALO_FP8_RB;
  *p = q;
  *chunk = ((byte % HALO_FP8_RB) >> 4) ^ halo_fp8_swz(q);
}

// element (= byte) offset into x (NHWC e4m3) of chunk `chunk` of patch
// pixel p of the tile at (b, ty0, tx0), or -1 = the zero page: outside the
// image (never the neighbouring row or image) or pad past the patch end
HALO_HD int64_t halo_fp8_src(const HaloGeo& g, int TH, int b, int ty0,
                             int tx0, int p, int chunk) {
  const int py = p / HALO_PW, px = p - py * HALO_PW;
  const int iy = ty0 - 1 + py, ix = tx0 - 1 + px;
  const bool ok = (p < halo_patch_px(TH)) & (iy >= 0) & (iy < g.H) &
                  (ix >= 0) & (ix < g.W);
  const int64_t off =
      ((int64_t)(b * g.H + iy) * g.W + ix) * g.Cin + chunk * HALO_FP8_EPC;
  return ok ? off : -1;
}

// byte address lane `lane` supplies to the ds_read_b128 of half `half`
// (0 = lo, channels 32*(l>>4) .. +15; 1 = hi, the next 16) of the fragment
// of tile row r, tap (dy, dx)
HALO_HD int halo_fp8_frag_off(int r, int dy, int dx, int half, int lane) {
  const int p = halo_frag_px(r, dy, dx) + (lane & 15);
  return halo_fp8_lds_off(p, 2 * (lane >> 4) + half);
}

// ------------------------------ wait counts ---------------------------------
// Issue order per wave: its patch pieces, the weight pieces of K-steps 0
// and 1, then in K-step s those of s + 2. The wait at the top of K-step s
// leaves only the newest step's pieces in flight.
HALO_HD int halo_fp8_wait_count(int step, int nsteps) {
  return step + 1 < nsteps ? HALO_FP8_WPIECES : 0;
}

// Weight stage: piece j of wave w holds rows (4j + w)*8 + (lane>>3) of the
// n block, lane-linear, the piece order of conv_mainloop_row128. The stage
// is laid out like the patch, byte(row, chunk) = halo_fp8_lds_off(row,
// chunk): lds_off_row128's chunk ^ (row & 7) is 2-way under the two-read
// fragment map (the host walk counts it), the patch swizzle is 1-way and
// repeats every 16 rows, so fragment ni stays a 2-KiB immediate. Returns
// the row and the SOURCE chunk of this lane's 16 B.
HALO_HD void halo_fp8_wpiece_slot(int j, int wid, int lane, int* row,
                                  int* chunk) {
  *row = (4 * j + wid) * 8 + (lane >> 3);
  *chunk = (lane & 7) ^ halo_fp8_swz(*row);
}

// byte address of half `half` of weight fragment ni = 0 for the wave
// column wc; fragment ni adds ni * 2048
HALO_HD int halo_fp8_wfrag_off(int wc, int half, int lane) {
  return halo_fp8_lds_off(wc * 64 + (lane & 15), 2 * (lane >> 4) + half);
}

}  // namespace rthd
