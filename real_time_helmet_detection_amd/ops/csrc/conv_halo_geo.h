// Geometry of the halo-tile 3x3 convs (conv_halo.hip, and with the traits
// of conv_halo_fp8_geo.h conv_halo_fp8.hip): the resident input patch in
// LDS, the piece -> source map of its global_load_lds fill, and the
// fragment-read offsets. Plain C++ with no HIP or torch dependency, so the
// same functions the kernel calls are walked lane by lane on the host
// (tests/conv_halo_geo_check.cpp) before anything runs on a GPU.
//
// A workgroup owns TH x 16 output pixels of one image (3x3, stride 1,
// pad 1). Its input patch is (TH+2) x 18 pixels, pixel p = py*18 + px at
// input (ty0 - 1 + py, tx0 - 1 + px), stored [p][Cin] with rows of
// RB bytes (bf16: 2*Cin, 256 B for Cin 128, 128 B for Cin 64; e4m3: 128 B)
// cut into 16-B channel chunks. In the bf16 kernel the A fragment of tap
// (dy, dx) for tile row r is one ds_read_b128 per lane: lane l reads pixel
// (r+dy)*18 + (l&15) + dx, chunk 4*kb + (l>>4) — the same lane -> (row,
// channel chunk) map as the per-tap tiles of conv.hip, with the tap folded
// into the start pixel.
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
constexpr int HALO_NBUF = 3;          // weight ring depth

struct HaloGeo {
  int B, H, W, Cin, Cout, Coutp;
  int tiles_y, tiles_x;  // H / TH, W / 16
};

HALO_HD int halo_patch_px(int TH) { return (TH + 2) * HALO_PW; }

// Per-dtype traits G of the patch image: RB bytes per patch pixel row, EPC
// elements per 16-B chunk, the XOR term swz(p) on the chunk index, and the
// weight ring stage (WSTAGE bytes, WPIECES 1-KiB pieces per wave per
// K-step). HaloBf16<CIN> is below, HaloFp8 in conv_halo_fp8_geo.h.
//
// The shifted fragment reads start at any patch pixel, so the XOR term
// must be 1-way for every run of 16 consecutive pixels. For the bf16
// kernel's one read per fragment (lane l: chunk 4*kb + (l>>4)):
//   256-B rows: the row term vanishes mod 64 banks; the 8 pixels of one
//     ds_read_b128 lane group that share a channel chunk are 8 distinct
//     values of p & 7, spread over chunk bits 1..3.
//   128-B rows: pixel parity picks the bank half, bits 1..2 of p spread
//     over chunk bits 1..2.
template <int CIN>
struct HaloBf16 {
  static constexpr int RB = CIN * 2;
  static constexpr int EPC = 8;
  static constexpr int WSTAGE = HALO_BN * 64;  // 128 rows x 32 ch
  static constexpr int WPIECES = 2;
  static HALO_HD int swz(int p) {
    return RB == 256 ? ((p & 7) << 1) : (((p >> 1) & 3) << 1);
  }
};

// 1-KiB pieces (one wave-instruction of 16 B per lane) that cover the
// patch; with 128-B rows the last piece may be half pad
template <typename G>
HALO_HD constexpr int halo_patch_pieces(int TH) {
  return ((TH + 2) * HALO_PW * G::RB + 1023) / 1024;
}

// LDS bytes of a block: the patch pieces and the weight ring
template <typename G>
HALO_HD constexpr int halo_lds_bytes(int TH) {
  return halo_patch_pieces<G>(TH) * 1024 + HALO_NBUF * G::WSTAGE;
}

// byte offset of 16-B channel chunk `chunk` of patch pixel p: the fill
// image and the read address both go through this one function
template <typename G>
HALO_HD int halo_lds_off(int p, int chunk) {
  return p * G::RB + ((chunk ^ G::swz(p)) << 4);
}

// Fill: piece f writes the lane-linear bytes [f*1024, f*1024 + 1024).
// Returns the patch pixel and the SOURCE channel chunk whose data must land
// at this lane's 16 B for the image to equal halo_lds_off's layout.
HALO_HD int halo_piece_byte(int f, int lane) { return f * 1024 + lane * 16; }

template <typename G>
HALO_HD void halo_piece_slot(int f, int lane, int* p, int* chunk) {
  const int byte = halo_piece_byte(f, lane);
  const int q = byte / G::RB;
  *p = q;
  *chunk = ((byte % G::RB) >> 4) ^ G::swz(q);
}

// element offset into x (NHWC) of channel chunk `chunk` of patch pixel p of
// the tile whose first output pixel is (b, ty0, tx0), or -1 = the zero
// page: outside the image (never the neighbouring row or image) or pad
// past the patch end
template <typename G>
HALO_HD int64_t halo_src(const HaloGeo& g, int TH, int b, int ty0, int tx0,
                         int p, int chunk) {
  const int py = p / HALO_PW, px = p - py * HALO_PW;
  const int iy = ty0 - 1 + py, ix = tx0 - 1 + px;
  const bool ok = (p < halo_patch_px(TH)) & (iy >= 0) & (iy < g.H) &
                  (ix >= 0) & (ix < g.W);
  const int64_t off =
      ((int64_t)(b * g.H + iy) * g.W + ix) * g.Cin + chunk * G::EPC;
  return ok ? off : -1;
}

// first patch pixel of the fragment of tile row r for tap (dy, dx) in
// 0..2 x 0..2; lane l reads pixel + (l & 15)
HALO_HD int halo_frag_px(int r, int dy, int dx) {
  return (r + dy) * HALO_PW + dx;
}

// byte address lane `lane` supplies to the bf16 kernel's ds_read_b128 for
// that fragment and 32-channel block kb. The kernel computes
// halo_frag_off(.., kb = 0) once per tap and XORs kb << 6 in: the chunk is
// (4*kb) ^ (l>>4) ^ swz bit by bit, and the pixel term has no bits below
// the row length.
template <typename G>
HALO_HD int halo_frag_off(int r, int dy, int dx, int kb, int lane) {
  const int p = halo_frag_px(r, dy, dx) + (lane & 15);
  return halo_lds_off<G>(p, 4 * kb + (lane >> 4));
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
template <typename G>
HALO_HD int halo_wait_count(int step, int nsteps) {
  return step + 1 < nsteps ? G::WPIECES : 0;
}

}  // namespace rthd
