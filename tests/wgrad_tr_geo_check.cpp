// Host walk of the transposed-read wgrad geometry (ops/csrc/wgrad_tr_geo.h).
// For every test shape it visits every lane of every staging
// and fragment-read instruction of every block, through the same functions
// the kernel calls, and checks that
//  1. every global source lies inside x / dy or is the zero page, and the
//     incremental pixel state equals the direct decomposition;
//  2. every LDS address is inside its tile and aligned (16 B stores, 8 B
//     reads), and the stores cover the tile exactly once;
//  3. stores and transposed reads compose to k = 8g + j, m = lane & 15;
//  4. the transposed reads are conflict-free per 32-lane half under the
//     64-bank rule (bank = (addr / 4) % 64); the ways are printed;
//  5. xcd_cell_remap is a permutation of 0 .. G - 1 for grid sizes G that
//     are and are not multiples of NUM_XCD, and one just above it.
// Exit status 0 = all checks passed.
#include "geo_check.h"
#include "wgrad_tr_geo.h"

using namespace rthd;

// LDS image checks of one operand tile of CH channels; fills inv[] with
// (row << 8 | channel) of every 2-byte element
static int check_tile_image(int CH, std::vector<int>* inv) {
  const int bytes = WTR_KB * CH * 2;
  const int nf = bytes / 1024;
  std::vector<int> hits(bytes / 16, 0);
  inv->assign(bytes / 2, -1);
  for (int f = 0; f < nf; ++f)
    for (int lane = 0; lane < 64; ++lane) {
      int row, chunk;
      wtr_stage_slot(f, lane, CH, &row, &chunk);
      const int addr = wtr_stage_byte(f, lane);
      CHECK(row >= 0 && row < WTR_KB && chunk >= 0 && chunk < CH / 8,
            "stage slot CH=%d f=%d lane=%d -> row %d chunk %d", CH, f, lane,
            row, chunk);
      CHECK(addr % 16 == 0 && addr + 16 <= bytes, "store addr %d", addr);
      CHECK(addr == wtr_lds_off(row, chunk, CH),
            "store image CH=%d row %d chunk %d: %d != %d", CH, row, chunk,
            addr, wtr_lds_off(row, chunk, CH));
      ++hits[addr / 16];
      for (int e = 0; e < 8; ++e)
        (*inv)[addr / 2 + e] = (row << 8) | (chunk * 8 + e);
    }
  for (int h : hits) CHECK(h == 1, "CH=%d: a 16-B slot stored %d times", CH, h);

  // transposed reads
  int worst = 0;
  for (int frag = 0; frag < CH / 16; ++frag)
    for (int ks = 0; ks < WTR_KB / 32; ++ks)
      for (int h = 0; h < 2; ++h) {
        int addr[64];
        for (int lane = 0; lane < 64; ++lane) {
          addr[lane] = wtr_tr_addr(frag, ks, h, lane, CH);
          CHECK(addr[lane] % 8 == 0 && addr[lane] >= 0 &&
                addr[lane] + 8 <= bytes, "read addr %d", addr[lane]);
        }
        char what[64];
        std::snprintf(what, sizeof what, "CH=%d frag %d ks %d", CH, frag, ks);
        tr_check_compose(addr, *inv, 32 * ks, h, 16 * frag, what);
        worst = std::max(worst, tr_read_ways(addr));
      }
  return worst;
}

struct Shape { int B, Cin, Cout, k, stride, pad, H, forced_chunk, min_steps; };

static void check_shape(const Shape& s, int BM, int BN) {
  WtrGeo g;
  g.B = s.B; g.H = s.H; g.W = s.H; g.Cin = s.Cin; g.Cout = s.Cout;
  g.KH = g.KW = s.k; g.stride = s.stride; g.pad = s.pad;
  g.Ho = (g.H + 2 * s.pad - s.k) / s.stride + 1;
  g.Wo = g.Ho;
  g.M = g.B * g.Ho * g.Wo;
  g.chunk_len = wtr_chunk_len(g.M, g.Cin, g.Cout, g.KH * g.KW,
                              s.forced_chunk);
  const int nchunks = cdiv(g.M, g.chunk_len);
  const int64_t xn = (int64_t)g.B * g.H * g.W * g.Cin;
  const int64_t yn = (int64_t)g.M * g.Cout;
  const int NX = WTR_KB * BM * 2 / 4096, NY = WTR_KB * BN * 2 / 4096;
  const int adv_b = WTR_KB / (g.Ho * g.Wo);
  const int adv_q = WTR_KB % (g.Ho * g.Wo) / g.Wo, adv_r = WTR_KB % g.Wo;
  long loads = 0, zeros = 0;
  int max_steps = 0;

  for (int chunk = 0; chunk < nchunks; ++chunk)
    for (int t = 0; t < g.KH * g.KW; ++t)
      for (int cit = 0; cit < cdiv(g.Cin, BM); ++cit)
        for (int cot = 0; cot < cdiv(g.Cout, BN); ++cot) {
          const int dyt = t / g.KW - g.pad, dxt = t % g.KW - g.pad;
          const int px_start = chunk * g.chunk_len;
          const int px_end = std::min(px_start + g.chunk_len, g.M);
          const int nsteps = cdiv(px_end - px_start, WTR_KB);
          CHECK(nsteps >= 1, "empty chunk %d", chunk);
          max_steps = std::max(max_steps, nsteps);
          for (int wid = 0; wid < 4; ++wid)
            for (int lane = 0; lane < 64; ++lane) {
              for (int i = 0; i < NX; ++i) {
                int row, c;
                wtr_stage_slot(i * 4 + wid, lane, BM, &row, &c);
                const int ch = cit * BM + c * 8;
                WtrPix pix;
                wtr_pix_init(px_start + row, g.Ho, g.Wo, &pix);
                for (int step = 0; step < nsteps; ++step) {
                  const int m = px_start + step * WTR_KB + row;
                  WtrPix ref;
                  wtr_pix_init(m, g.Ho, g.Wo, &ref);
                  CHECK(pix.b == ref.b && pix.oy == ref.oy && pix.ox == ref.ox,
                        "pixel walk m=%d: (%d,%d,%d) != (%d,%d,%d)", m, pix.b,
                        pix.oy, pix.ox, ref.b, ref.oy, ref.ox);
                  const int64_t off =
                      wtr_x_src(g, pix, m, px_end, dyt, dxt, ch);
                  ++loads;
                  if (off < 0) {
                    ++zeros;
                  } else {
                    CHECK(off + 8 <= xn && off % 8 == 0, "x source %lld of "
                          "%lld", (long long)off, (long long)xn);
                    const int iy = ref.oy * g.stride + dyt;
                    const int ix = ref.ox * g.stride + dxt;
                    CHECK(m < g.M && off == (((int64_t)ref.b * g.H + iy) *
                                             g.W + ix) * g.Cin + ch,
                          "x source map m=%d", m);
                  }
                  wtr_pix_advance(&pix, adv_b, adv_q, adv_r, g.Ho, g.Wo);
                }
              }
              for (int i = 0; i < NY; ++i) {
                int row, c;
                wtr_stage_slot(i * 4 + wid, lane, BN, &row, &c);
                const int ch = cot * BN + c * 8;
                for (int step = 0; step < nsteps; ++step) {
                  const int m = px_start + step * WTR_KB + row;
                  const int64_t off = wtr_dy_src(g, m, px_end, ch);
                  ++loads;
                  if (off < 0) ++zeros;
                  else CHECK(off + 8 <= yn && off % 8 == 0 &&
                             off == (int64_t)m * g.Cout + ch,
                             "dy source %lld of %lld", (long long)off,
                             (long long)yn);
                }
              }
            }
        }
  std::printf("shape B%d %d->%d k%d s%d p%d H%d chunk %d (%d K-steps) tile "
              "%dx%d: %ld loads, %ld zero-page\n", s.B, s.Cin, s.Cout, s.k,
              s.stride, s.pad, s.H, g.chunk_len, max_steps, BM, BN, loads,
              zeros);
  CHECK(max_steps >= s.min_steps, "shape meant to run >= %d K-steps runs %d",
        s.min_steps, max_steps);
}

static void check_xcd_remap(int G) {
  std::vector<int> hits(G, 0);
  for (int cell = 0; cell < G; ++cell) {
    const int c = xcd_cell_remap(cell, G);
    CHECK(c >= 0 && c < G, "G=%d: block %d -> cell %d", G, cell, c);
    if (c >= 0 && c < G) ++hits[c];
  }
  for (int c = 0; c < G; ++c)
    CHECK(hits[c] == 1, "G=%d: cell %d is taken %d times", G, c, hits[c]);
}

int main() {
  for (int G : {8, 9, 15, 64, 509, 4608}) check_xcd_remap(G);
  std::vector<int> inv;
  for (int CH : {64, 128}) {
    const int ways = check_tile_image(CH, &inv);
    std::printf("tile [%d px][%d ch]: transposed-read conflict ways per "
                "32-lane half = %d\n", WTR_KB, CH, ways);
    CHECK(ways == 1, "CH=%d transposed reads are %d-way", CH, ways);
  }
  const Shape shapes[] = {
      // the GPU test shapes at the default chunk (128 px: 1-2 K-steps)
      {2, 64, 32, 3, 1, 1, 12, 0, 1},   {2, 128, 128, 3, 1, 1, 16, 0, 1},
      {2, 128, 128, 1, 1, 0, 16, 0, 1}, {2, 64, 128, 3, 1, 1, 16, 0, 1},
      {2, 152, 64, 1, 1, 0, 32, 0, 1},  {2, 128, 8, 1, 1, 0, 16, 0, 1},
      {1, 128, 128, 3, 1, 1, 8, 0, 1},  {2, 128, 128, 2, 2, 0, 16, 0, 1},
      {2, 128, 128, 3, 1, 1, 16, 128, 1},
      // many K-steps per chunk: the ring wraps, the pixel walk advances
      // many times. 12^2 = 144 and 20^2 = 400 px per image are no divisors
      // or multiples of the 64-px K-step; the 1x1 takes the 2048-px rule.
      {2, 128, 128, 3, 1, 1, 16, 512, 8}, {4, 64, 32, 3, 1, 1, 12, 512, 8},
      {3, 72, 136, 3, 1, 1, 20, 1024, 16}, {2, 152, 64, 1, 1, 0, 64, 0, 32},
      {3, 64, 64, 3, 2, 1, 40, 640, 10},  {16, 8, 8, 3, 1, 1, 64, 0, 10},
  };
  // the tile the kernel is instantiated at (wgrad_tr.hip: WTR_BM x WTR_BN)
  for (const Shape& s : shapes) check_shape(s, 64, 128);
  return geo_report();
}
