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

// The traits of conv_halo_geo.h for the e4m3 patch. XOR term on the 3-bit
// chunk index: one ds_read_b128 of a fragment half takes the chunks
// {h, 2+h, 4+h, 6+h} of 16 consecutive pixels from any start. HaloBf16's
// swizzle is 2-way under that map, this one is 1-way (bit 2 of p picks
// chunk bit 0, bit 1 of p chunk bit 2; the host walk is the proof).
struct HaloFp8 {
  static constexpr int RB = 128;   // patch row bytes
  static constexpr int EPC = 16;   // e4m3 elements per 16-B chunk
  static constexpr int WSTAGE = HALO_BN * 128;  // 128 rows x 128 B
  static constexpr int WPIECES = 4;
  static HALO_HD int swz(int p) {
    return ((p >> 2) & 1) | (((p >> 1) & 1) << 2);
  }
};

// byte address lane `lane` supplies to the ds_read_b128 of half `half`
// (0 = lo, channels 32*(l>>4) .. +15; 1 = hi, the next 16) of the fragment
// of tile row r, tap (dy, dx)
HALO_HD int halo_fp8_frag_off(int r, int dy, int dx, int half, int lane) {
  const int p = halo_frag_px(r, dy, dx) + (lane & 15);
  return halo_lds_off<HaloFp8>(p, 2 * (lane >> 4) + half);
}

// Weight stage: piece j of wave w holds rows (4j + w)*8 + (lane>>3) of the
// n block, lane-linear, the piece order of conv_mainloop_row128. The stage
// is laid out like the patch, byte(row, chunk) = halo_lds_off<HaloFp8>(
// row, chunk): lds_off_row128's chunk ^ (row & 7) is 2-way under the two-read
// fragment map (the host walk counts it), the patch swizzle is 1-way and
// repeats every 16 rows, so fragment ni stays a 2-KiB immediate. Returns
// the row and the SOURCE chunk of this lane's 16 B.
HALO_HD void halo_fp8_wpiece_slot(int j, int wid, int lane, int* row,
                                  int* chunk) {
  *row = (4 * j + wid) * 8 + (lane >> 3);
  *chunk = (lane & 7) ^ HaloFp8::swz(*row);
}

// byte address of half `half` of weight fragment ni = 0 for the wave
// column wc; fragment ni adds ni * 2048
HALO_HD int halo_fp8_wfrag_off(int wc, int half, int lane) {
  return halo_lds_off<HaloFp8>(wc * 64 + (lane & 15), 2 * (lane >> 4) + half);
}

}  // namespace rthd
