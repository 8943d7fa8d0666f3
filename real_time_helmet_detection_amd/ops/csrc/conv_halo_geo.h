// Geometry of the halo-tile 3x3 bf16 conv (conv_halo.hip): the resident
// input patch in LDS, the piece -> source map of its global_load_lds fill,
// and the fragment-read offsets. Plain C++ with no HIP or torch dependency,
// so the same functions the kernel calls are walked lane by lane on the
// host (tests/conv_halo_geo_check.cpp) before anything runs on a GPU.
//
// A workgroup owns TH x 16 output pixels of one image (3x3, stride 1,
// pad 1). Its input patch is (TH+2) x 18 pixels, pixel p = py*18 + px at
// input (ty0 - 1 + py, tx0 - 1 + px), stored [p][Cin] with rows of
// RB = 2*Cin bytes (256 B for Cin 128, 128 B for Cin 64) cut into 16-B
// channel chunks. The A fragment of tap (dy, dx) for tile row r is one
// ds_read_b128 per lane: lane l reads pixel (r+dy)*18 + (l&15) + dx,
// chunk 4*kb + (l>>4) — the same lane -> (row, channel chunk) map as the
// per-tap tiles of conv.hip, with the tap folded into the start pixel.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define HALO_HD __host__ __device__ inline
#else
#define HALO_HD inline
#endif

namespace rthd {

constexpr int HALO_TW = 16;           // tile width: one fragment = one row
constexpr int HALO_PW = HALO_TW + 2;  // patch width
constexpr int HALO_BN = 128;          // output channels per workgroup
constexpr int HALO_WSTAGE = HALO_BN * 64;  // weight ring stage: 128 x 32 ch
constexpr int HALO_NBUF = 3;          // weight ring depth
constexpr int HALO_WPIECES = 2;       // weight pieces per wave per K-step

struct HaloGeo {
  int B, H, W, Cin, Cout, Coutp;
  int tiles_y, tiles_x;  // H / TH, W / 16
};

HALO_HD int halo_patch_px(int TH) { return (TH + 2) * HALO_PW; }

// 1-KiB pieces (one wave-instruction of 16 B per lane) that cover the
// patch; with 128-B rows the last piece is half pad
HALO_HD int halo_patch_pieces(int TH, int RB) {
  return (halo_patch_px(TH) * RB + 1023) / 1024;
}

// The shifted fragment reads start at any patch pixel, so the XOR term
// must be 1-way for every run of 16 consecutive pixels:
//   256-B rows: the row term vanishes mod 64 banks; the 8 pixels of one
//     ds_read_b128 lane group that share a channel chunk are 8 distinct
//     values of p & 7, spread over chunk bits 1..3.
//   128-B rows: pixel parity picks the bank half, bits 1..2 of p spread
//     over chunk bits 1..2.
HALO_HD int halo_swz(int p, int RB) {
  return RB == 256 ? ((p & 7) << 1) : (((p >> 1) & 3) << 1);
}

// byte offset of 16-B channel chunk `chunk` of patch pixel p: the fill
// image and the read address both go through this one function
HALO_HD int halo_lds_off(int p, int chunk, int RB) {
  return p * RB + ((chunk ^ halo_swz(p, RB)) << 4);
}

// Fill: piece f writes the lane-linear bytes [f*1024, f*1024 + 1024).
// Returns the patch pixel and the SOURCE channel chunk whose data must land
// at this lane's 16 B for the image to equal halo_lds_off's layout.
HALO_HD int halo_piece_byte(int f, int lane) { return f * 1024 + lane * 16; }

HALO_HD void halo_piece_slot(int f, int lane, int RB, int* p, int* chunk) {
  const int byte = halo_piece_byte(f, lane);
  const int q = byte / RB;
  *p = q;
  *chunk = ((byte % RB) >> 4) ^ halo_swz(q, RB);
}

// element offset into x (NHWC) of channel chunk `chunk` of patch pixel p of
// the tile whose first output pixel is (b, ty0, tx0), or -1 = the zero
// page: outside the image (never the neighbouring row or image) or pad
// past the patch end
HALO_HD int64_t halo_src(const HaloGeo& g, int TH, int b, int ty0, int tx0,
                         int p, int chunk) {
  const int py = p / HALO_PW, px = p - py * HALO_PW;
  const int iy = ty0 - 1 + py, ix = tx0 - 1 + px;
  const bool ok = (p < halo_patch_px(TH)) & (iy >= 0) & (iy < g.H) &
                  (ix >= 0) & (ix < g.W);
  const int64_t off =
      ((int64_t)(b * g.H + iy) * g.W + ix) * g.Cin + chunk * 8;
  return ok ? off : -1;
}

// first patch pixel of the fragment of tile row r for tap (dy, dx) in
// 0..2 x 0..2; lane l reads pixel + (l & 15)
HALO_HD int halo_frag_px(int r, int dy, int dx) {
  return (r + dy) * HALO_PW + dx;
}

// byte address lane `lane` supplies to ds_read_b128 for that fragment and
// 32-channel block kb. The kernel computes halo_frag_off(.., kb = 0) once
// per tap and XORs kb << 6 in: the chunk is (4*kb) ^ (l>>4) ^ swz bit by
// bit, and the pixel term has no bits below the row length.
HALO_HD int halo_frag_off(int r, int dy, int dx, int kb, int lane, int RB) {
  const int p = halo_frag_px(r, dy, dx) + (lane & 15);
  return halo_lds_off(p, 4 * kb + (lane >> 4), RB);
}

// block id -> (n block, batch, tile origin); the n blocks of one tile are
// neighbours. (The XCD block remap of wgrad_tr measured neutral here and
// is not used: profiles/conv_halo.md.)
HALO_HD void halo_cell_decompose(const HaloGeo& g, int TH, int cell,
                                 int* nblk, int* b, int* ty0, int* tx0) {
  const int nn = g.Coutp / HALO_BN;
  *nblk = cell % nn;
  int t = cell / nn;
  *tx0 = (t % g.tiles_x) * HALO_TW;
  t /= g.tiles_x;
  *ty0 = (t % g.tiles_y) * TH;
  *b = t / g.tiles_y;
}

// ------------------------------ wait counts ---------------------------------
// Every wave issues, in order: its patch pieces, the weight pieces of
// K-step 0, those of K-step 1, and then in K-step s those of s + 2. vmcnt
// retires in issue order, so the wait at the top of K-step s leaves only
// the newest step's pieces in flight: patch and weights of s have landed.
HALO_HD int halo_wait_count(int step, int nsteps) {
  return step + 1 < nsteps ? HALO_WPIECES : 0;
}

}  // namespace rthd
