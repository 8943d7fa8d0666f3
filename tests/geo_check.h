// Shared pieces of the host geometry walks (tests/*_geo_check.cpp): the
// CHECK macro with its failure counter and final report, and the LDS bank
// models of the two fragment-read instructions.
#pragma once

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

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

// the last lines of main(): the exit status
static inline int geo_report() {
  if (g_fail) {
    std::printf("%d checks FAILED\n", g_fail);
    return 1;
  }
  std::printf("all geometry checks passed\n");
  return 0;
}

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// worst number of distinct addresses on one of the 64 banks
// (bank = (addr / 4) % 64) when lanes[0..n) each read `dwords` dwords
static inline int bank_ways(const int* addr, const int* lanes, int n,
                            int dwords) {
  std::vector<std::vector<int>> on_bank(64);
  for (int i = 0; i < n; ++i)
    for (int d = 0; d < dwords; ++d) {
      const int a = addr[lanes[i]] + 4 * d;
      auto& v = on_bank[(a / 4) % 64];
      if (std::find(v.begin(), v.end(), a) == v.end()) v.push_back(a);
    }
  int worst = 0;
  for (auto& v : on_bank) worst = std::max(worst, (int)v.size());
  return worst;
}

// ---- ds_read_b128: the lanes of a wave are served in four groups
static const int kGroups[4][16] = {
    {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
    {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
    {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
    {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};

// conflict ways of one ds_read_b128 wave-instruction
static inline int read_ways(const int* addr) {
  int worst = 0;
  for (int grp = 0; grp < 4; ++grp)
    worst = std::max(worst, bank_ways(addr, kGroups[grp], 16, 4));
  return worst;
}

// ---- ds_read_b64_tr_b16: 8 B per lane, served per 32-lane half

// conflict ways of one transposed-read wave-instruction
static inline int tr_read_ways(const int* addr) {
  int lanes[32], worst = 0;
  for (int half = 0; half < 2; ++half) {
    for (int l = 0; l < 32; ++l) lanes[l] = half * 32 + l;
    worst = std::max(worst, bank_ways(addr, lanes, 32, 2));
  }
  return worst;
}

// The hardware gather of one transposed read of half h (k-slots j = 4h ..
// 4h + 3): lane i of 16-lane group g receives as element q column i of the
// row whose address lanes 4q .. 4q+3 of the group supply. inv[] maps every
// 2-byte LDS element to (row << 8 | channel); the read must deliver row
// row0 + 8g + j, channel ch0 + i. `what` names the read in a failure.
static inline void tr_check_compose(const int* addr,
                                    const std::vector<int>& inv, int row0,
                                    int h, int ch0, const char* what) {
  for (int lane = 0; lane < 64; ++lane) {
    const int g = lane >> 4, i = lane & 15;
    for (int q = 0; q < 4; ++q) {
      const int a = addr[16 * g + 4 * q + (i >> 2)] + 2 * (i & 3);
      const int got = inv[a / 2];
      const int j = 4 * h + q;
      const int want = ((row0 + 8 * g + j) << 8) | (ch0 + i);
      CHECK(got == want, "compose %s lane %d j %d: row %d ch %d, want row %d "
            "ch %d", what, lane, j, got >> 8, got & 255, want >> 8,
            want & 255);
    }
  }
}
