// Host walk of the halo-tile conv geometry (ops/csrc/conv_halo_geo.h).
// For every GPU test shape, both tile heights and both row lengths it
// visits every lane of every patch piece and every fragment read of every
// block, through the same functions the kernel calls, and checks that
//  1. every patch byte is written by exactly one lane of one piece, inside
//     the LDS the kernel allocates, and lands where halo_lds_off says;
//  2. every source is the right pixel and chunk of the block's own image,
//     and every out-of-image pixel (and the pad past the patch) is the zero
//     page: never the neighbouring row, image or batch entry;
//  3. every fragment read, for all 9 taps, tile rows and K blocks, returns
//     input pixel (y + dy - 1, x + dx - 1), channels 32 kb + 8 (l >> 4) ..,
//     and the kernel's XOR form of the K block equals halo_frag_off;
//  4. every fragment read is 1-way under the ds_read_b128 lane groups
//     {0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32 (64 banks);
//  5. blocks cover every output tile of every image exactly once;
//  6. replaying the issue order (patch pieces, weights of K-steps 0 and 1,
//     then step s + 2 in step s) against halo_wait_count leaves exactly the
//     newest step's weight pieces in flight at each wait, and a ring buffer
//     is refilled only after the step that read it.
// 1, 2, 5 and 6 are the walks of halo_geo_check.h.
// Exit status 0 = all checks passed.
#include "halo_geo_check.h"

// image and read checks that do not depend on the tensor shape
template <typename G>
static void check_image(int TH) {
  const int RB = G::RB;
  const int ppx = halo_patch_px(TH);
  const int np = halo_patch_pieces<G>(TH);
  const int bytes = np * 1024;
  std::vector<int> inv;
  halo_check_fill<G>(TH, &inv);

  int worst = 0;
  for (int r = 0; r < TH; ++r)
    for (int dy = 0; dy < 3; ++dy)
      for (int dx = 0; dx < 3; ++dx)
        for (int kb = 0; kb < RB / 64; ++kb) {
          int addr[64];
          for (int lane = 0; lane < 64; ++lane) {
            addr[lane] = halo_frag_off<G>(r, dy, dx, kb, lane);
            CHECK(addr[lane] % 16 == 0 && addr[lane] >= 0 &&
                  addr[lane] + 16 <= bytes, "read addr %d", addr[lane]);
            // the kernel's form: kb = 0 offset, kb XORed into bits 6..7
            CHECK(addr[lane] ==
                  (halo_frag_off<G>(r, dy, dx, 0, lane) ^ (kb << 6)),
                  "XOR form r%d tap(%d,%d) kb%d lane%d", r, dy, dx, kb, lane);
            const int want_p = (r + dy) * HALO_PW + (lane & 15) + dx;
            const int want_c = 4 * kb + (lane >> 4);
            CHECK(want_p < ppx && inv[addr[lane] / 16] == want_p * 16 + want_c,
                  "fragment r%d tap(%d,%d) kb%d lane%d reads p %d chunk %d, "
                  "wants p %d chunk %d", r, dy, dx, kb, lane,
                  inv[addr[lane] / 16] / 16, inv[addr[lane] / 16] % 16,
                  want_p, want_c);
          }
          worst = std::max(worst, read_ways(addr));
        }
  std::printf("tile %dx16, %d-B rows: %d px patch, %d pieces, fragment-read "
              "conflict ways = %d\n", TH, RB, ppx, np, worst);
  CHECK(worst == 1, "TH%d RB%d fragment reads are %d-way", TH, RB, worst);
}

template <typename G>
static void check_shape(const Shape& s, int TH) {
  if (s.H % TH || s.W % HALO_TW) {
    std::printf("shape B%d %d->%d %dx%d: no %dx16 tiling (the kernel "
                "refuses it)\n", s.B, s.Cin, s.Cout, s.H, s.W, TH);
    return;
  }
  halo_check_shape<G>(s, TH);
}

int main() {
  for (int TH : {8, 16}) {
    check_image<HaloBf16<64>>(TH);
    check_image<HaloBf16<128>>(TH);
    halo_check_waits<HaloBf16<64>>(TH, 9 * 2);   // NSTEPS = 9 * Cin / 32
    halo_check_waits<HaloBf16<128>>(TH, 9 * 4);
  }
  const Shape shapes[] = {
      // the GPU test shapes
      {2, 128, 128, 16, 32}, {3, 64, 128, 8, 16}, {2, 128, 64, 24, 48},
      {1, 128, 128, 12, 20}, {1, 64, 40, 8, 16}, {1, 128, 40, 8, 16},
      {1, 64, 44, 8, 16}, {1, 128, 44, 8, 16},
      // the same at twice the height (what a 16-row tile needs), an odd
      // block count, two n blocks
      {2, 128, 128, 32, 32}, {3, 64, 128, 16, 16}, {2, 128, 64, 48, 48},
      {5, 64, 64, 8, 48}, {1, 128, 256, 16, 16},
  };
  for (const Shape& s : shapes)
    for (int TH : {8, 16}) {
      if (s.Cin == 64) check_shape<HaloBf16<64>>(s, TH);
      else             check_shape<HaloBf16<128>>(s, TH);
    }
  return geo_report();
}
