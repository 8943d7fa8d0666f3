// The walks the two halo-tile geometry checks share (conv_halo_geo_check.cpp,
// conv_halo_fp8_geo_check.cpp), over the traits G of conv_halo_geo.h: the
// patch fill image, the per-shape source map and block cover, and the
// issue-order replay of the wait counts. The fragment reads differ per
// kernel and stay in the two programs.
#pragma once

#include "conv_halo_geo.h"
#include "geo_check.h"
#include "lds_ring.h"

using namespace rthd;

// Fill image of a TH x 16 tile: every patch byte is written by exactly one
// lane of one piece, inside the LDS the kernel allocates, and lands where
// halo_lds_off says. inv[] maps every 16-B slot to p * 16 + chunk.
template <typename G>
static void halo_check_fill(int TH, std::vector<int>* inv_out) {
  const int RB = G::RB;
  const int ppx = halo_patch_px(TH);
  const int np = halo_patch_pieces<G>(TH);
  const int bytes = np * 1024;
  const int cpr = RB / 16;  // chunks per row
  std::vector<int> hits(bytes / 16, 0);
  std::vector<int>& inv = *inv_out;
  inv.assign(bytes / 16, -1);
  for (int f = 0; f < np; ++f)
    for (int lane = 0; lane < 64; ++lane) {
      int p, c;
      halo_piece_slot<G>(f, lane, &p, &c);
      const int addr = halo_piece_byte(f, lane);
      CHECK(addr % 16 == 0 && addr >= 0 && addr + 16 <= bytes,
            "piece addr %d of %d", addr, bytes);
      CHECK(c >= 0 && c < cpr && p >= 0, "slot TH%d RB%d f%d lane%d -> p %d "
            "chunk %d", TH, RB, f, lane, p, c);
      if (p < ppx)
        CHECK(addr == halo_lds_off<G>(p, c), "image TH%d RB%d p %d chunk %d:"
              " %d != %d", TH, RB, p, c, addr, halo_lds_off<G>(p, c));
      ++hits[addr / 16];
      inv[addr / 16] = p * 16 + c;
    }
  for (int h : hits) CHECK(h == 1, "a 16-B slot is written %d times", h);
  for (int p = 0; p < ppx; ++p)
    for (int c = 0; c < cpr; ++c) {
      const int a = halo_lds_off<G>(p, c);
      CHECK(a >= 0 && a + 16 <= bytes && inv[a / 16] == p * 16 + c,
            "patch p %d chunk %d has no writer", p, c);
    }
}

struct Shape { int B, Cin, Cout, H, W; };

// Per shape: blocks cover every output tile of every image exactly once;
// every source is the right pixel and chunk of the block's own image, and
// every out-of-image pixel (and the pad past the patch) is the zero page.
template <typename G>
static void halo_check_shape(const Shape& s, int TH) {
  HaloGeo g;
  g.B = s.B; g.H = s.H; g.W = s.W; g.Cin = s.Cin; g.Cout = s.Cout;
  g.Coutp = (s.Cout + 127) / 128 * 128;
  g.tiles_y = s.H / TH;
  g.tiles_x = s.W / HALO_TW;
  const int EPC = G::EPC;
  const int np = halo_patch_pieces<G>(TH);
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
        halo_piece_slot<G>(f, lane, &p, &c);
        const int64_t off = halo_src<G>(g, TH, b, ty0, tx0, p, c);
        const int iy = ty0 - 1 + p / HALO_PW, ix = tx0 - 1 + p % HALO_PW;
        const bool inside = p < halo_patch_px(TH) && iy >= 0 && iy < g.H &&
                            ix >= 0 && ix < g.W;
        ++loads;
        if (off < 0) ++zeros;
        CHECK((off >= 0) == inside, "zero-page rule b%d tile(%d,%d) p %d: "
              "off %lld, pixel (%d,%d)", b, ty0, tx0, p, (long long)off, iy,
              ix);
        if (off >= 0)
          CHECK(off % EPC == 0 && off + EPC <= xn &&
                off == (((int64_t)b * g.H + iy) * g.W + ix) * g.Cin + c * EPC,
                "source b%d tile(%d,%d) p %d chunk %d: %lld of %lld", b,
                ty0, tx0, p, c, (long long)off, (long long)xn);
      }
  }
  for (int v : seen) CHECK(v == 1, "a tile is computed %d times", v);
  std::printf("shape B%d %d->%d %dx%d tile %dx16: %d blocks, %ld loads, %ld "
              "zero-page\n", s.B, s.Cin, s.Cout, s.H, s.W, TH, nblocks, loads,
              zeros);
}

// Issue-order replay of one wave's vmcnt queue (patch pieces, weights of
// K-steps 0 and 1, then step s + 2 in step s) against halo_wait_count: each
// wait leaves exactly the newest step's weight pieces in flight, and a ring
// buffer is refilled only after the step that read it.
template <typename G>
static void halo_check_waits(int TH, int nsteps) {
  for (int wid = 0; wid < 4; ++wid) {
    std::vector<int> q;  // tag per outstanding piece: -1 patch, else K-step
    for (int f = wid; f < halo_patch_pieces<G>(TH); f += 4) q.push_back(-1);
    for (int i = 0; i < G::WPIECES; ++i) q.push_back(0);
    for (int i = 0; i < G::WPIECES; ++i) q.push_back(1);
    CHECK((int)q.size() <= 63, "more pieces queued than vmcnt counts");
    int ring[HALO_NBUF] = {0, 1, -1};  // K-step whose weights a buffer holds
    int rbuf = 0;
    for (int step = 0; step < nsteps; ++step) {
      const int n = halo_wait_count<G>(step, nsteps);
      CHECK((int)q.size() >= n, "step %d waits for more than is queued", step);
      while ((int)q.size() > n) q.erase(q.begin());  // retires oldest first
      for (int tag : q)
        CHECK(tag == step + 1, "step %d: piece of %d still in flight", step,
              tag);
      CHECK((int)q.size() == (step + 1 < nsteps ? G::WPIECES : 0),
            "step %d leaves %d pieces in flight", step, (int)q.size());
      CHECK(ring[rbuf] == step, "step %d reads buffer %d holding step %d",
            step, rbuf, ring[rbuf]);
      const int wbuf = ring3_prev(rbuf);
      if (step + 2 < nsteps) {
        // refilled after the barrier of this step: its last reader was
        // step - 1, whose reads were waited for before that barrier
        CHECK(ring[wbuf] == step - 1 || ring[wbuf] == -1,
              "step %d refills buffer %d holding step %d", step, wbuf,
              ring[wbuf]);
        ring[wbuf] = step + 2;
        for (int i = 0; i < G::WPIECES; ++i) q.push_back(step + 2);
      }
      rbuf = ring3_next(rbuf);
    }
    CHECK(q.empty(), "pieces in flight at the end");
  }
}
