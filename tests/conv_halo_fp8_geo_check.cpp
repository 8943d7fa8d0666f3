// Host walk of the halo-tile fp8 conv geometry
// (ops/csrc/conv_halo_fp8_geo.h). For every GPU test shape it visits every
// lane of every patch piece and every fragment read of every block, through
// the same functions the kernel calls, and checks that
//  1. every patch byte is written by exactly one lane of one piece, inside
//     the LDS the kernel allocates, and lands where halo_fp8_lds_off says;
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
//     then step s + 2 in step s) against halo_fp8_wait_count leaves exactly
//     the newest step's weight pieces in flight at each wait, and a ring
//     buffer is refilled only after the step that read it.
// Exit status 0 = all checks passed.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "conv_halo_fp8_geo.h"

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
static void check_image(int TH) {
  const int RB = HALO_FP8_RB;
  const int ppx = halo_patch_px(TH);
  const int np = halo_fp8_patch_pieces(TH);
  const int bytes = np * 1024;
  const int cpr = RB / 16;  // chunks per row
  std::vector<int> hits(bytes / 16, 0), inv(bytes / 16, -1);
  for (int f = 0; f < np; ++f)
    for (int lane = 0; lane < 64; ++lane) {
      int p, c;
      halo_fp8_piece_slot(f, lane, &p, &c);
      const int addr = halo_piece_byte(f, lane);
      CHECK(addr % 16 == 0 && addr >= 0 && addr + 16 <= bytes,
            "piece addr %d of %d", addr, bytes);
      CHECK(c >= 0 && c < cpr && p >= 0, "slot TH%d f%d lane%d -> p %d "
            "chunk %d", TH, f, lane, p, c);
      if (p < ppx)
        CHECK(addr == halo_fp8_lds_off(p, c), "image TH%d p %d chunk %d:"
              " %d != %d", TH, p, c, addr, halo_fp8_lds_off(p, c));
      ++hits[addr / 16];
      inv[addr / 16] = p * 16 + c;
    }
  for (int h : hits) CHECK(h == 1, "a 16-B slot is written %d times", h);
  for (int p = 0; p < ppx; ++p)
    for (int c = 0; c < cpr; ++c) {
      const int a = halo_fp8_lds_off(p, c);
      CHECK(a >= 0 && a + 16 <= bytes && inv[a / 16] == p * 16 + c,
            "patch p %d chunk %d has no writer", p, c);
    }

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
  auto off128 = [](int row, int chunk) { return halo_fp8_lds_off(row, chunk); };
  {
    int addr[64];
    for (int lane = 0; lane < 64; ++lane) {
      const int row = lane & 15, chunk = 2 * (lane >> 4);
      addr[lane] = row * 128 + ((chunk ^ (row & 7)) << 4);
    }
    std::printf("weight stage in chunk ^ (row & 7) layout: %d-way (not "
                "used)\n", read_ways(addr));
  }
  std::vector<int> hits(HALO_FP8_WSTAGE / 16, 0);
  for (int wid = 0; wid < 4; ++wid)
    for (int j = 0; j < HALO_FP8_WPIECES; ++j)
      for (int lane = 0; lane < 64; ++lane) {
        int row, c;
        halo_fp8_wpiece_slot(j, wid, lane, &row, &c);
        const int addr = (4 * j + wid) * 1024 + lane * 16;
        CHECK(row >= 0 && row < HALO_BN && c >= 0 && c < 8,
              "weight slot j%d w%d lane%d -> row %d chunk %d", j, wid, lane,
              row, c);
        CHECK(addr + 16 <= HALO_FP8_WSTAGE && addr == off128(row, c),
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

struct Shape { int B, Cin, Cout, H, W; };

static void check_shape(const Shape& s, int TH) {
  if (s.H % TH || s.W % HALO_TW || s.Cin != HALO_FP8_CIN) {
    std::printf("shape B%d %d->%d %dx%d: no %dx16 tiling or Cin != 128 (the "
                "kernel refuses it)\n", s.B, s.Cin, s.Cout, s.H, s.W, TH);
    return;
  }
  HaloGeo g;
  g.B = s.B; g.H = s.H; g.W = s.W; g.Cin = s.Cin; g.Cout = s.Cout;
  g.Coutp = (s.Cout + 127) / 128 * 128;
  g.tiles_y = s.H / TH;
  g.tiles_x = s.W / HALO_TW;
  const int np = halo_fp8_patch_pieces(TH);
  const int64_t xn = (int64_t)s.B * s.H * s.W * s.Cin;
  const int nblocks = g.B * g.tiles_y * g.tiles_x * (g.Coutp / HALO_BN);
  long loads = 0, zeros = 0;
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
        halo_fp8_piece_slot(f, lane, &p, &c);
        const int64_t off = halo_fp8_src(g, TH, b, ty0, tx0, p, c);
        const int iy = ty0 - 1 + p / HALO_PW, ix = tx0 - 1 + p % HALO_PW;
        const bool inside = p < halo_patch_px(TH) && iy >= 0 && iy < g.H &&
                            ix >= 0 && ix < g.W;
        ++loads;
        if (off < 0) ++zeros;
        CHECK((off >= 0) == inside, "zero-page rule b%d tile(%d,%d) p %d: "
              "off %lld, pixel (%d,%d)", b, ty0, tx0, p, (long long)off, iy,
              ix);
        if (off >= 0)
          CHECK(off % 16 == 0 && off + 16 <= xn &&
                off == (((int64_t)b * g.H + iy) * g.W + ix) * g.Cin + c * 16,
                "source b%d tile(%d,%d) p %d chunk %d: %lld of %lld", b,
                ty0, tx0, p, c, (long long)off, (long long)xn);
      }
  }
  for (int v : seen) CHECK(v == 1, "a tile is computed %d times", v);
  std::printf("shape B%d %d->%d %dx%d tile %dx16: %d blocks, %ld loads, %ld "
              "zero-page\n", s.B, s.Cin, s.Cout, s.H, s.W, TH, nblocks, loads,
              zeros);
}

// issue-order replay of one wave's vmcnt queue
static void check_waits(int TH) {
  const int nsteps = 9;
  for (int wid = 0; wid < 4; ++wid) {
    std::vector<int> q;  // tag per outstanding piece: -1 patch, else K-step
    for (int f = wid; f < halo_fp8_patch_pieces(TH); f += 4) q.push_back(-1);
    for (int i = 0; i < HALO_FP8_WPIECES; ++i) q.push_back(0);
    for (int i = 0; i < HALO_FP8_WPIECES; ++i) q.push_back(1);
    CHECK((int)q.size() <= 63, "more pieces queued than vmcnt counts");
    int ring[HALO_FP8_NBUF] = {0, 1, -1};  // K-step a buffer holds
    int rbuf = 0;
    for (int step = 0; step < nsteps; ++step) {
      const int n = halo_fp8_wait_count(step, nsteps);
      CHECK((int)q.size() >= n, "step %d waits for more than is queued", step);
      while ((int)q.size() > n) q.erase(q.begin());  // retires oldest first
      for (int tag : q)
        CHECK(tag == step + 1, "step %d: piece of %d still in flight", step,
              tag);
      CHECK((int)q.size() == (step + 1 < nsteps ? HALO_FP8_WPIECES : 0),
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
        for (int i = 0; i < HALO_FP8_WPIECES; ++i) q.push_back(step + 2);
      }
      rbuf = rbuf == 2 ? 0 : rbuf + 1;
    }
    CHECK(q.empty(), "pieces in flight at the end");
  }
}

int main() {
  for (int TH : {8, 16}) {
    check_image(TH);
    check_waits(TH);
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
  if (g_fail) {
    std::printf("%d checks FAILED\n", g_fail);
    return 1;
  }
  std::printf("all geometry checks passed\n");
  return 0;
}
