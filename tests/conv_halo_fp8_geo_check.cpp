// Host walk of the halo-tile fp8 conv geometry
// (ops/csrc/conv_halo_fp8_geo.h). For every GPU test shape it visits every
// lane of every patch piece and every fragment read of every block, through
// the same functions the kernel calls, and checks that
//  1. every patch byte is written by exactly one lane of one piece, inside
//     the LDS the kernel allocates, and lands where halo_lds_off<HaloFp8> says;
//  2. every source is the right pixel and chunk of the block's own image,
//     and every out-of-image pixel (and the pad past the patch) is the zero
//     page: never the neighbouring row, image or batch entry;
//  3. both halves of every fragment read, for all 9 taps and tile rows,
//     return input pixel (y + dy - 1, x + dx - 1), channels
//     32 (l >> 4) + 16 half .., and the kernel's XOR form of the half
//     equals halo_fp8_frag_off;
//  4. every fragment read is 1-way under the ds_read_b128 lane groups
//     {0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32 (64 banks);
//     so is every weight fragment read of the 128-B-row stage;
//  5. blocks cover every output tile of every image exactly once;
//  6. the weight pieces of the four waves cover the 16-KB stage exactly
//     once in the 128-B-row swizzled layout;
//  7. replaying the issue order (patch pieces, weights of K-steps 0 and 1,
//     then step s + 2 in step s) against halo_wait_count leaves exactly
//     the newest step's weight pieces in flight at each wait, and a ring
//     buffer is refilled only after the step that read it.
// 1, 2, 5 and 7 are the walks of halo_geo_check.h.
// Exit status 0 = all checks passed.
#include "conv_halo_fp8_geo.h"
#include "halo_geo_check.h"

// image and read checks that do not depend on the tensor shape
static void check_image(int TH) {
  const int ppx = halo_patch_px(TH);
  const int np = halo_patch_pieces<HaloFp8>(TH);
  const int bytes = np * 1024;
  std::vector<int> inv;
  halo_check_fill<HaloFp8>(TH, &inv);

  int worst = 0;
  for (int r = 0; r < TH; ++r)
    for (int dy = 0; dy < 3; ++dy)
      for (int dx = 0; dx < 3; ++dx)
        for (int half = 0; half < 2; ++half) {
          int addr[64];
          for (int lane = 0; lane < 64; ++lane) {
            addr[lane] = halo_fp8_frag_off(r, dy, dx, half, lane);
            CHECK(addr[lane] % 16 == 0 && addr[lane] >= 0 &&
                  addr[lane] + 16 <= bytes, "read addr %d", addr[lane]);
            // the kernel's form: the lo offset with the half XORed into
            // bit 4
            CHECK(addr[lane] ==
                  (halo_fp8_frag_off(r, dy, dx, 0, lane) ^ (half << 4)),
                  "XOR form r%d tap(%d,%d) half%d lane%d", r, dy, dx, half,
                  lane);
            const int want_p = (r + dy) * HALO_PW + (lane & 15) + dx;
            const int want_c = 2 * (lane >> 4) + half;
            CHECK(want_p < ppx && inv[addr[lane] / 16] == want_p * 16 + want_c,
                  "fragment r%d tap(%d,%d) half%d lane%d reads p %d chunk %d, "
                  "wants p %d chunk %d", r, dy, dx, half, lane,
                  inv[addr[lane] / 16] / 16, inv[addr[lane] / 16] % 16,
                  want_p, want_c);
          }
          worst = std::max(worst, read_ways(addr));
        }
  std::printf("tile %dx16, 128-B rows: %d px patch, %d pieces, fragment-read "
              "conflict ways = %d\n", TH, ppx, np, worst);
  CHECK(worst == 1, "TH%d fragment reads are %d-way", TH, worst);
}

// the weight stage: 4 pieces per wave cover [128 rows][128 B] once, in the
// layout the B fragment reads (row wc*64 + 16 ni + (l & 15), chunks
// 2*(l>>4) + half) expect; those reads are 1-way. For the record it also
// counts the ways of the 128x128 kernel's chunk ^ (row & 7) layout.
static void check_weight_stage() {
  auto off128 = [](int row, int chunk) {
    return halo_lds_off<HaloFp8>(row, chunk);
  };
  {
    int addr[64];
    for (int lane = 0; lane < 64; ++lane) {
      const int row = lane & 15, chunk = 2 * (lane >> 4);
      addr[lane] = row * 128 + ((chunk ^ (row & 7)) << 4);
    }
    std::printf("weight stage in chunk ^ (row & 7) layout: %d-way (not "
                "used)\n", read_ways(addr));
  }
  std::vector<int> hits(HaloFp8::WSTAGE / 16, 0);
  for (int wid = 0; wid < 4; ++wid)
    for (int j = 0; j < HaloFp8::WPIECES; ++j)
      for (int lane = 0; lane < 64; ++lane) {
        int row, c;
        halo_fp8_wpiece_slot(j, wid, lane, &row, &c);
        const int addr = (4 * j + wid) * 1024 + lane * 16;
        CHECK(row >= 0 && row < HALO_BN && c >= 0 && c < 8,
              "weight slot j%d w%d lane%d -> row %d chunk %d", j, wid, lane,
              row, c);
        CHECK(addr + 16 <= HaloFp8::WSTAGE && addr == off128(row, c),
              "weight image row %d chunk %d: %d != %d", row, c, addr,
              off128(row, c));
        ++hits[addr / 16];
      }
  for (int h : hits) CHECK(h == 1, "a weight slot is written %d times", h);
  int worst = 0;
  for (int wc = 0; wc < 2; ++wc)
    for (int ni = 0; ni < 4; ++ni)
      for (int half = 0; half < 2; ++half) {
        int addr[64];
        for (int lane = 0; lane < 64; ++lane) {
          addr[lane] = off128(wc * 64 + 16 * ni + (lane & 15),
                              2 * (lane >> 4) + half);
          // the kernel's form: ni as a 2-KiB immediate
          CHECK(addr[lane] == halo_fp8_wfrag_off(wc, half, lane) + ni * 2048,
                "weight read form wc%d ni%d half%d lane%d", wc, ni, half,
                lane);
        }
        worst = std::max(worst, read_ways(addr));
      }
  std::printf("weight stage: fragment-read conflict ways = %d\n", worst);
  CHECK(worst == 1, "weight fragment reads are %d-way", worst);
}

static void check_shape(const Shape& s, int TH) {
  if (s.H % TH || s.W % HALO_TW || s.Cin != HALO_FP8_CIN) {
    std::printf("shape B%d %d->%d %dx%d: no %dx16 tiling or Cin != 128 (the "
                "kernel refuses it)\n", s.B, s.Cin, s.Cout, s.H, s.W, TH);
    return;
  }
  halo_check_shape<HaloFp8>(s, TH);
}

int main() {
  for (int TH : {8, 16}) {
    check_image(TH);
    halo_check_waits<HaloFp8>(TH, 9);
  }
  check_weight_stage();
  const Shape shapes[] = {
      // the GPU test shapes
      {2, 128, 128, 16, 32}, {3, 128, 64, 8, 16}, {1, 128, 256, 24, 48},
      {1, 128, 40, 8, 16},
      // the refused ones, and the routed serving shapes' tiling in small
      {1, 128, 128, 12, 20}, {1, 256, 128, 16, 32}, {4, 128, 128, 64, 64},
      {5, 128, 64, 8, 48},
  };
  for (const Shape& s : shapes) check_shape(s, 8);
  return geo_report();
}
