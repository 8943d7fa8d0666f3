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
// Exit status 0 = all checks passed.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "conv_halo_geo.h"

using namespace rthd;

static int g_fail = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (g_fail < 20) {                                  \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__);  \
        std::printf(__VA_ARGS__);                         \
        std::printf("\n");                                \
      }                                                   \
      ++g_fail;                                           \
    }                                                     \
  } while (0)

static const int kGroups[4][16] = {
    {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
    {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
    {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
    {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};

// conflict ways of one ds_read_b128 wave-instruction
static int read_ways(const int* addr) {
  int worst = 0;
  for (int grp = 0; grp < 4; ++grp) {
    std::vector<std::vector<int>> on_bank(64);
    for (int i = 0; i < 16; ++i)
      for (int d = 0; d < 4; ++d) {
        const int a = addr[kGroups[grp][i]] + 4 * d;
        auto& v = on_bank[(a / 4) % 64];
        if (std::find(v.begin(), v.end(), a) == v.end()) v.push_back(a);
      }
    for (auto& v : on_bank) worst = std::max(worst, (int)v.size());
  }
  return worst;
}

// image and read checks that do not depend on the tensor shape
static void check_image(int TH, int RB) {
  const int ppx = halo_patch_px(TH);
  const int np = halo_patch_pieces(TH, RB);
  const int bytes = np * 1024;
  const int cpr = RB / 16;  // chunks per row
  std::vector<int> hits(bytes / 16, 0), inv(bytes / 16, -1);
  for (int f = 0; f < np; ++f)
    for (int lane = 0; lane < 64; ++lane) {
      int p, c;
      halo_piece_slot(f, lane, RB, &p, &c);
      const int addr = halo_piece_byte(f, lane);
      CHECK(addr % 16 == 0 && addr >= 0 && addr + 16 <= bytes,
            "piece addr %d of %d", addr, bytes);
      CHECK(c >= 0 && c < cpr && p >= 0, "slot TH%d RB%d f%d lane%d -> p %d "
            "chunk %d", TH, RB, f, lane, p, c);
      if (p < ppx)
        CHECK(addr == halo_lds_off(p, c, RB), "image TH%d RB%d p %d chunk %d:"
              " %d != %d", TH, RB, p, c, addr, halo_lds_off(p, c, RB));
      ++hits[addr / 16];
      inv[addr / 16] = p * 16 + c;
    }
  for (int h : hits) CHECK(h == 1, "a 16-B slot is written %d times", h);
  for (int p = 0; p < ppx; ++p)
    for (int c = 0; c < cpr; ++c) {
      const int a = halo_lds_off(p, c, RB);
      CHECK(a >= 0 && a + 16 <= bytes && inv[a / 16] == p * 16 + c,
            "patch p %d chunk %d has no writer", p, c);
    }

  int worst = 0;
  for (int r = 0; r < TH; ++r)
    for (int dy = 0; dy < 3; ++dy)
      for (int dx = 0; dx < 3; ++dx)
        for (int kb = 0; kb < RB / 64; ++kb) {
          int addr[64];
          for (int lane = 0; lane < 64; ++lane) {
            addr[lane] = halo_frag_off(r, dy, dx, kb, lane, RB);
            CHECK(addr[lane] % 16 == 0 && addr[lane] >= 0 &&
                  addr[lane] + 16 <= bytes, "read addr %d", addr[lane]);
            // the kernel's form: kb = 0 offset, kb XORed into bits 6..7
            CHECK(addr[lane] ==
                  (halo_frag_off(r, dy, dx, 0, lane, RB) ^ (kb << 6)),
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

struct Shape { int B, Cin, Cout, H, W; };

static void check_shape(const Shape& s, int TH) {
  if (s.H % TH || s.W % HALO_TW) {
    std::printf("shape B%d %d->%d %dx%d: no %dx16 tiling (the kernel "
                "refuses it)\n", s.B, s.Cin, s.Cout, s.H, s.W, TH);
    return;
  }
  HaloGeo g;
  g.B = s.B; g.H = s.H; g.W = s.W; g.Cin = s.Cin; g.Cout = s.Cout;
  g.Coutp = (s.Cout + 127) / 128 * 128;
  g.tiles_y = s.H / TH;
  g.tiles_x = s.W / HALO_TW;
  const int RB = s.Cin * 2;
  const int np = halo_patch_pieces(TH, RB);
  const int64_t xn = (int64_t)s.B * s.H * s.W * s.Cin;
  const int nblocks = g.B * g.tiles_y * g.tiles_x * (g.Coutp / HALO_BN);
  long loads = 0, zeros = 0;
  {
    std::vector<int> seen(nblocks, 0);
    for (int cell = 0; cell < nblocks; ++cell) {
      int nblk, b, ty0, tx0;
      halo_cell_decompose(g, TH, cell, &nblk, &b, &ty0, &tx0);
      const int id = ((b * g.tiles_y + ty0 / TH) * g.tiles_x +
                      tx0 / HALO_TW) * (g.Coutp / HALO_BN) + nblk;
      CHECK(nblk >= 0 && nblk < g.Coutp / HALO_BN && b >= 0 && b < g.B &&
            ty0 >= 0 && ty0 + TH <= g.H && ty0 % TH == 0 && tx0 >= 0 &&
            tx0 + HALO_TW <= g.W && tx0 % HALO_TW == 0,
            "cell %d -> n%d b%d (%d,%d)", cell, nblk, b, ty0, tx0);
      if (id >= 0 && id < nblocks) ++seen[id];
      for (int f = 0; f < np; ++f)
        for (int lane = 0; lane < 64; ++lane) {
          int p, c;
          halo_piece_slot(f, lane, RB, &p, &c);
          const int64_t off = halo_src(g, TH, b, ty0, tx0, p, c);
          const int iy = ty0 - 1 + p / HALO_PW, ix = tx0 - 1 + p % HALO_PW;
          const bool inside = p < halo_patch_px(TH) && iy >= 0 && iy < g.H &&
                              ix >= 0 && ix < g.W;
          ++loads;
          if (off < 0) ++zeros;
          CHECK((off >= 0) == inside, "zero-page rule b%d tile(%d,%d) p %d: "
                "off %lld, pixel (%d,%d)", b, ty0, tx0, p, (long long)off, iy,
                ix);
          if (off >= 0)
            CHECK(off % 8 == 0 && off + 8 <= xn &&
                  off == (((int64_t)b * g.H + iy) * g.W + ix) * g.Cin + c * 8,
                  "source b%d tile(%d,%d) p %d chunk %d: %lld of %lld", b,
                  ty0, tx0, p, c, (long long)off, (long long)xn);
        }
    }
    for (int v : seen) CHECK(v == 1, "a tile is computed %d times", v);
  }
  std::printf("shape B%d %d->%d %dx%d tile %dx16: %d blocks, %ld loads, %ld "
              "zero-page\n", s.B, s.Cin, s.Cout, s.H, s.W, TH, nblocks, loads,
              zeros);
}

// issue-order replay of one wave's vmcnt queue
static void check_waits(int TH, int RB) {
  const int nsteps = 9 * (RB / 64);
  for (int wid = 0; wid < 4; ++wid) {
    std::vector<int> q;  // tag per outstanding piece: -1 patch, else K-step
    for (int f = wid; f < halo_patch_pieces(TH, RB); f += 4) q.push_back(-1);
    for (int i = 0; i < HALO_WPIECES; ++i) q.push_back(0);
    for (int i = 0; i < HALO_WPIECES; ++i) q.push_back(1);
    int ring[HALO_NBUF] = {0, 1, -1};  // K-step whose weights a buffer holds
    int rbuf = 0;
    for (int step = 0; step < nsteps; ++step) {
      const int n = halo_wait_count(step, nsteps);
      CHECK((int)q.size() >= n, "step %d waits for more than is queued", step);
      while ((int)q.size() > n) q.erase(q.begin());  // retires oldest first
      for (int tag : q)
        CHECK(tag == step + 1, "step %d: piece of %d still in flight", step,
              tag);
      CHECK((int)q.size() == (step + 1 < nsteps ? HALO_WPIECES : 0),
            "step %d leaves %d pieces in flight", step, (int)q.size());
      CHECK(ring[rbuf] == step, "step %d reads buffer %d holding step %d",
            step, rbuf, ring[rbuf]);
      const int wbuf = rbuf == 0 ? 2 : rbuf - 1;
      if (step + 2 < nsteps) {
        // refilled after the barrier of this step: its last reader was
        // step - 1, whose reads were waited for before that barrier
        CHECK(ring[wbuf] == step - 1 || ring[wbuf] == -1,
              "step %d refills buffer %d holding step %d", step, wbuf,
              ring[wbuf]);
        ring[wbuf] = step + 2;
        for (int i = 0; i < HALO_WPIECES; ++i) q.push_back(step + 2);
      }
      rbuf = rbuf == 2 ? 0 : rbuf + 1;
    }
    CHECK(q.empty(), "pieces in flight at the end");
  }
}

int main() {
  for (int TH : {8, 16})
    for (int RB : {128, 256}) {
      check_image(TH, RB);
      check_waits(TH, RB);
    }
  const Shape shapes[] = {
      // the GPU test shapes
      {2, 128, 128, 16, 32}, {3, 64, 128, 8, 16}, {2, 128, 64, 24, 48},
      {1, 128, 128, 12, 20},
      // the same at twice the height (what a 16-row tile needs), an odd
      // block count, two n blocks
      {2, 128, 128, 32, 32}, {3, 64, 128, 16, 16}, {2, 128, 64, 48, 48},
      {5, 64, 64, 8, 48}, {1, 128, 256, 16, 16},
  };
  for (const Shape& s : shapes)
    for (int TH : {8, 16}) check_shape(s, TH);
  if (g_fail) {
    std::printf("%d checks FAILED\n", g_fail);
    return 1;
  }
  std::printf("all geometry checks passed\n");
  return 0;
}
