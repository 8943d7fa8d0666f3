// Host walk of the tap-row wgrad geometry (ops/csrc/wgrad_row_geo.h), through
// the functions the kernel calls. It checks that
//  1. the X fill image (every staged piece, apron and filler rows included)
//     is inside the stage, covers it once and equals the read map: the
//     shifted transposed reads of tap dx deliver k-slot (g, j), channel
//     16 frag + i from LDS row apron + 32 ks + 8 g + j + dx;
//  2. those reads are 1-way per 32-lane half under the 64-bank rule for all
//     three shifts, both row widths, every fragment, k-block and half;
//  3. per shape and block, every X source is the zero page or lies inside
//     x, inside [0, M), inside the batch entry and image row the pixel
//     belongs to, and is real data wherever a tap needs it; the pixel walk
//     equals the direct decomposition;
//  4. the register masks hit exactly the ox == 0 (tap -1) and ox == Wo - 1
//     (tap +1) pixels for Wo in {32, 64, 128, 256} and every chunk start;
//  5. the chunk rule gives multiples of 128.
// Exit status 0 = all checks passed.
#include "geo_check.h"
#include "wgrad_row_geo.h"

using namespace rthd;

// X image of CH channels: fill vs shifted reads, and the conflict ways
static int check_x_image(int CH) {
  const int np = wrow_x_pieces(CH), rows = wrow_x_rows(CH);
  const int bytes = np * 1024;
  CHECK(rows >= WROW_USED && rows * CH * 2 == bytes, "CH=%d: %d rows", CH,
        rows);
  int owned = 0;
  for (int w = 0; w < 4; ++w) owned += wrow_x_wave_pieces(w, CH);
  CHECK(owned == np, "CH=%d: waves own %d of %d pieces", CH, owned, np);
  std::vector<int> hits(bytes / 16, 0), inv(bytes / 2, -1);
  for (int f = 0; f < np; ++f)
    for (int lane = 0; lane < 64; ++lane) {
      int row, chunk;
      wtr_stage_slot(f, lane, CH, &row, &chunk);
      const int addr = wtr_stage_byte(f, lane);
      CHECK(row >= 0 && row < rows && chunk >= 0 && chunk < CH / 8,
            "stage slot CH=%d f=%d lane=%d -> row %d chunk %d", CH, f, lane,
            row, chunk);
      CHECK(addr % 16 == 0 && addr + 16 <= bytes, "store addr %d", addr);
      CHECK(addr == wtr_lds_off(row, chunk, CH), "store image CH=%d row %d",
            CH, row);
      ++hits[addr / 16];
      for (int e = 0; e < 8; ++e)
        inv[addr / 2 + e] = (row << 8) | (chunk * 8 + e);
    }
  for (int h : hits) CHECK(h == 1, "CH=%d: a 16-B slot stored %d times", CH, h);

  int worst = 0;
  for (int dx = -1; dx <= 1; ++dx)
    for (int frag = 0; frag < CH / 16; ++frag)
      for (int ks = 0; ks < WTR_KB / 32; ++ks)
        for (int h = 0; h < 2; ++h) {
          int addr[64];
          for (int lane = 0; lane < 64; ++lane) {
            addr[lane] = wrow_tr_addr(frag, ks, h, dx, lane, CH);
            CHECK(addr[lane] % 8 == 0 && addr[lane] >= 0 &&
                  addr[lane] + 8 <= bytes, "read addr %d", addr[lane]);
            // k-block 1 is read with an offset immediate of 32 rows
            CHECK(ks == 0 || addr[lane] == wrow_tr_addr(frag, 0, h, dx, lane,
                                                        CH) + 32 * CH * 2,
                  "k-block 1 is not k-block 0 + 32 rows");
          }
          char what[64];
          std::snprintf(what, sizeof what, "CH=%d dx %d frag %d ks %d", CH,
                        dx, frag, ks);
          tr_check_compose(addr, inv, WROW_APRON + dx + 32 * ks, h, 16 * frag,
                           what);
          worst = std::max(worst, tr_read_ways(addr));
        }
  return worst;
}

struct Shape { int Cin, Cout, H, W, B, forced_chunk, min_steps; };

static void check_shape(const Shape& s, int BM, int BN) {
  WtrGeo g;
  g.B = s.B; g.H = s.H; g.W = s.W; g.Cin = s.Cin; g.Cout = s.Cout;
  g.KH = g.KW = 3; g.stride = 1; g.pad = 1;
  g.Ho = g.H; g.Wo = g.W;
  g.M = g.B * g.Ho * g.Wo;
  CHECK(wrow_eligible(g), "shape not eligible");
  g.chunk_len = wrow_chunk_len(g.M, g.Cin, g.Cout, s.forced_chunk);
  CHECK(g.chunk_len % 128 == 0 && g.chunk_len >= 128, "chunk %d",
        g.chunk_len);
  const int nchunks = cdiv(g.M, g.chunk_len);
  const int64_t xn = (int64_t)g.B * g.H * g.W * g.Cin;
  const int np = wrow_x_pieces(BM);
  const int adv_b = WTR_KB / (g.Ho * g.Wo);
  const int adv_q = WTR_KB % (g.Ho * g.Wo) / g.Wo, adv_r = WTR_KB % g.Wo;
  long loads = 0, zeros = 0;
  int max_steps = 0;

  for (int chunk = 0; chunk < nchunks; ++chunk)
    for (int ty = 0; ty < 3; ++ty)
      for (int cit = 0; cit < cdiv(g.Cin, BM); ++cit) {
        const int dyt = ty - 1;
        const int px_start = chunk * g.chunk_len;
        const int px_end = std::min(px_start + g.chunk_len, g.M);
        const int nsteps = cdiv(px_end - px_start, WTR_KB);
        CHECK(nsteps >= 1, "empty chunk %d", chunk);
        max_steps = std::max(max_steps, nsteps);
        for (int wid = 0; wid < 4; ++wid)
          for (int lane = 0; lane < 64; ++lane)
            for (int i = 0; i < wrow_x_wave_pieces(wid, BM); ++i) {
              CHECK(i * 4 + wid < np, "piece %d of wave %d", i, wid);
              int row, c;
              wtr_stage_slot(i * 4 + wid, lane, BM, &row, &c);
              const int ch = cit * BM + c * 8;
              WtrPix pix;
              wrow_pix_init(px_start - WROW_APRON + row, g.Ho, g.Wo, &pix);
              for (int step = 0; step < nsteps; ++step) {
                const int p0 = px_start + step * WTR_KB;
                const int m = p0 - WROW_APRON + row;
                if (m >= 0) {
                  WtrPix ref;
                  wtr_pix_init(m, g.Ho, g.Wo, &ref);
                  CHECK(pix.b == ref.b && pix.oy == ref.oy &&
                        pix.ox == ref.ox, "pixel walk m=%d: (%d,%d,%d) != "
                        "(%d,%d,%d)", m, pix.b, pix.oy, pix.ox, ref.b, ref.oy,
                        ref.ox);
                }
                const int64_t off =
                    wrow_x_src(g, pix, m, row, px_end, dyt, ch);
                ++loads;
                // is this (pixel, channel) real data some tap needs?
                // tap dx of output pixel q < px_end reads pixel q + dx,
                // unless masked (edge) or out of the image rows
                bool needed = false;
                if (m >= 0 && m < g.M && ch < g.Cin && row < WROW_USED) {
                  const int oy = m / g.Wo % g.Ho;
                  const bool row_in = oy + dyt >= 0 && oy + dyt < g.H;
                  for (int dx = -1; dx <= 1; ++dx) {
                    const int q = m - dx;   // the output pixel that reads m
                    const int slot = row - WROW_APRON - dx;
                    if (slot < 0 || slot >= WTR_KB) continue;
                    if (q < p0 || q >= px_end) continue;
                    const int qx = q % g.Wo;
                    if (qx + dx < 0 || qx + dx >= g.Wo) continue;   // masked
                    if (row_in) needed = true;
                  }
                }
                if (off < 0) {
                  ++zeros;
                  CHECK(!needed, "needed pixel m=%d row %d is the zero page",
                        m, row);
                } else {
                  CHECK(off + 8 <= xn && off % 8 == 0, "x source %lld of "
                        "%lld", (long long)off, (long long)xn);
                  CHECK(m >= 0 && m < g.M, "source for pixel %d outside "
                        "[0, M)", m);
                  const int b = m / (g.Ho * g.Wo), oy = m / g.Wo % g.Ho;
                  const int ox = m % g.Wo, iy = oy + dyt;
                  CHECK(iy >= 0 && iy < g.H, "source row %d outside the "
                        "image", iy);
                  CHECK(off == (((int64_t)b * g.H + iy) * g.W + ox) * g.Cin +
                               ch, "x source map m=%d", m);
                }
                wtr_pix_advance(&pix, adv_b, adv_q, adv_r, g.Ho, g.Wo);
              }
            }
      }
  std::printf("shape B%d %d->%d %dx%d chunk %d (%d K-steps) tile 3x%dx%d: "
              "%ld X loads, %ld zero-page\n", s.B, s.Cin, s.Cout, s.H, s.W,
              g.chunk_len, max_steps, BM, BN, loads, zeros);
  CHECK(max_steps >= s.min_steps, "shape meant to run >= %d K-steps runs %d",
        s.min_steps, max_steps);
}

// the masks as the kernel applies them: the set of masked k-slots of the
// 32-px k-block starting at pixel p equals the edge pixels
static void check_masks(int Wo) {
  const int Ho = 4, M = 3 * Ho * Wo;
  for (int start = 0; start < M; start += 128) {
    // the kernel's walk of the step's first ox from the chunk start
    int oxs = start % Wo;
    for (int p0 = start; p0 < M; p0 += WTR_KB) {
      for (int ks = 0; ks < 2; ++ks) {
        int oxk = oxs + 32 * ks;
        oxk -= oxk >= Wo ? Wo : 0;
        const int p = p0 + 32 * ks;
        CHECK(oxk == p % Wo, "ox walk at pixel %d: %d", p, oxk);
        for (int dx = -1; dx <= 1; ++dx)
          for (int lane = 0; lane < 64; ++lane)
            for (int h = 0; h < 2; ++h)
              for (int reg = 0; reg < 2; ++reg) {
                uint32_t word = 0xffffffffu;
                if (h == wrow_mask_half(dx) && reg == wrow_mask_reg(dx) &&
                    wrow_edge(dx, oxk, Wo))
                  word = wrow_mask_word(dx, lane);
                for (int e = 0; e < 2; ++e) {
                  const int j = 4 * h + 2 * reg + e;
                  const int px = p + 8 * (lane >> 4) + j;
                  const int ox = px % Wo;
                  const bool masked = ((word >> (16 * e)) & 0xffffu) == 0;
                  const bool part = ((word >> (16 * e)) & 0xffffu) != 0xffffu;
                  const bool want = (dx < 0 && ox == 0) ||
                                    (dx > 0 && ox == Wo - 1);
                  CHECK(masked == want && part == want, "Wo %d pixel %d dx "
                        "%d: masked %d, want %d", Wo, px, dx, masked, want);
                }
              }
      }
      oxs += WTR_KB % Wo;
      oxs -= oxs >= Wo ? Wo : 0;
    }
  }
}

int main() {
  for (int CH : {64, 128}) {
    const int ways = check_x_image(CH);
    std::printf("X image [%d px][%d ch]: shifted transposed-read conflict "
                "ways per 32-lane half = %d\n", wrow_x_rows(CH), CH, ways);
    CHECK(ways == 1, "CH=%d shifted reads are %d-way", CH, ways);
  }
  for (int Wo : {32, 64, 128, 256}) check_masks(Wo);
  // chunk rule: multiples of 128 for the step's shapes and odd sizes
  for (int M : {4224, 16384, 65536, 262144, 1048576, 3 * 24 * 64})
    for (int C : {64, 72, 128, 136, 256}) {
      const int len = wrow_chunk_len(M, C, C, 0);
      CHECK(len >= 128 && len % 128 == 0, "chunk rule M=%d C=%d: %d", M, C,
            len);
      CHECK(wrow_chunk_len(M, C, C, 200) == 256, "forced chunk rounds up");
    }
  const Shape shapes[] = {
      // the GPU test shapes
      {64, 64, 8, 32, 2, 0, 1},       {128, 128, 32, 32, 2, 512, 8},
      {64, 128, 24, 64, 3, 1024, 16}, {72, 136, 8, 64, 2, 0, 1},
      {128, 128, 2, 256, 2, 128, 2},  {64, 64, 4, 64, 2, 0, 1},
      // Wo no power of two; an image of 96 px rows
      {64, 64, 5, 96, 3, 256, 4},
  };
  for (const Shape& s : shapes) {
    check_shape(s, 64, 128);   // the tile wgrad_row.hip is instantiated at
    check_shape(s, 128, 64);
  }
  return geo_report();
}
