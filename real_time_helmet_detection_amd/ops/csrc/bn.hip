// Training-mode BatchNorm kernels (NHWC) + column reduction (conv dbias).
//
// The fused conv epilogue can fold BN only in inference (running stats);
// training needs batch stats of the conv output, so the training path is
//   conv(linear epilogue) -> bn_stats -> bn_act_fwd     [3 kernels]
// Backward: one reduce kernel (d_beta = sum dpre, d_gamma = sum dpre*xhat)
// + one apply kernel for dx, where dpre = dy * act'(pre) is recomputed from
// the saved conv output and stats — no extra saved activations.
//
// Reduction design (the first version used per-channel atomicAdd from every
// block: ~2k same-address atomic RMWs serialize to ~250 us per call):
// blocks write per-chunk PARTIALS; the last blocks to arrive sum the
// [chunks][C] partials in a fixed order, in the same launch ("ticket" path;
// RTHD_BN_STAGED=1 selects the older finish by two further tiny launches) —
// contention-free AND deterministic.
//
// bf16 kernels use the row-interleaved octet mapping: thread t owns channel
// octet t%octs across rows t/octs + k*streams, so a wave reads contiguous
// full rows (16 B/lane, no over-fetch — guide G13) and per-channel
// parameters hoist out of the row loop. Requires octs = C/8 a power of two;
// anything else falls back to the scalar generic path.
//
// Dual form (a Residual whose skip is conv+BN): y = act(bn(x) + bf16(bn_s(xs)))
// in ONE forward pass and one reduce + one apply pass backward, in place of
// the skip BN's own three kernels; the normalised skip s and its gradient
// never reach memory. Both are rounded in registers exactly where their
// stores rounded them, and every sum keeps its chunking, its stream walk and
// its finish, so the results are bitwise those of the separate kernels.
//
// Layout of this file: each mapping (scalar, octet) has ONE reduce skeleton
// and ONE apply shell; what a kernel computes is a small functor handed to
// the skeleton as its first argument.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <map>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>
#include "common.h"

namespace rthd {

// per-channel fp32 vectors every BN kernel reads
struct BnParams {
  const float *mean, *rstd, *gamma, *beta;
};

// The BN(+skip)+act backward expression tree, written once. The order —
// (x-mu)*rsd, then xh*gm+bt, then +skip, then dy*act' — and the compiler's
// default fp contraction of it are part of the kernels' bitwise contract.
struct BnGrad {
  float xh, pre, dpre;
};

template <bool HAS_SKIP>
DEV_INLINE BnGrad bn_grad(float x, float mu, float rsd, float gm, float bt,
                          float skip, float dy, int act) {
  const float xh = (x - mu) * rsd;
  float pre = xh * gm + bt;
  if (HAS_SKIP) pre += skip;
  return {xh, pre, dy * act_grad_by_sign(pre, act)};
}

// 16 B of bf16 <-> bf16[8]
DEV_INLINE void ld8(bf16 (&v)[8], const bf16* p) {
  *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(p);
}
DEV_INLINE void st8(bf16* p, const bf16 (&v)[8]) {
  *reinterpret_cast<uint4*>(p) = *reinterpret_cast<const uint4*>(v);
}

// the four parameter vectors of one channel octet, hoisted into registers
struct BnOct {
  float mu[8], rsd[8], gm[8], bt[8];
};

DEV_INLINE BnOct load_oct(const BnParams& p, int c0) {
  BnOct o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    o.mu[e] = p.mean[c0 + e];
    o.rsd[e] = p.rstd[c0 + e];
    o.gm[e] = p.gamma[c0 + e];
    o.bt[e] = p.beta[c0 + e];
  }
  return o;
}

// value of v after a store to T and a load back
template <typename T> DEV_INLINE float round_as(float v);
template <> DEV_INLINE float round_as<float>(float v) { return v; }
template <> DEV_INLINE float round_as<bf16>(float v) { return b2f(f2b(v)); }

// The skip tensor of the dual kernels, as the forward kernel of the same
// mapping wrote it (Linear act): the scalar kernels use the unfolded
// expression, the octet kernels the folded scale/shift one.
template <typename T>
DEV_INLINE float bn_skip_elem(float xs, float mu, float rsd, float gm,
                              float bt) {
  const float xh = (xs - mu) * rsd;
  return round_as<T>(xh * gm + bt);
}

struct BnFold {
  float sc[8], sh[8];
};

DEV_INLINE BnFold fold_oct(const BnParams& p, int c0) {
  BnFold f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float g = p.gamma[c0 + e] * p.rstd[c0 + e];
    f.sc[e] = g;
    f.sh[e] = p.beta[c0 + e] - p.mean[c0 + e] * g;
  }
  return f;
}

DEV_INLINE float bn_skip_oct(float xs, float sc, float sh) {
  return b2f(f2b(xs * sc + sh));
}

// number of column groups ("pairs" of sums) a reduce functor carries: the
// dual functors say kPairs = 2 and see virtual columns [0, 2C), the second C
// of them being the skip BN's
template <typename F, typename = void>
struct reduce_pairs {
  static constexpr int value = 1;
};
template <typename F>
struct reduce_pairs<F, std::void_t<decltype(F::kPairs)>> {
  static constexpr int value = F::kPairs;
};

// fixed-order sum of the 4 sub-streams of a 64-channel x 4 block
DEV_INLINE float sum4(const float* sh) {
  return sh[threadIdx.x] + sh[threadIdx.x + 64] + sh[threadIdx.x + 128] +
         sh[threadIdx.x + 192];
}

static bool fast8_ok(const torch::Tensor& t, int C) {
  const int octs = C / 8;
  return t.scalar_type() == at::kBFloat16 && C % 8 == 0 && octs > 0 &&
         octs <= 256 && (octs & (octs - 1)) == 0;
}

static int pick_chunks(int64_t M, int C) {
  // enough blocks to fill 256 CUs (a 256 cap left 1 block/CU -> 1.5 TB/s)
  int64_t chunks = cdiv((int64_t)M * C, (int64_t)16384);
  if (chunks > 1024) chunks = 1024;
  if (chunks < 1) chunks = 1;
  return (int)chunks;
}

// ----------------------------- reduce functors ------------------------------
// Reduce functors add one element (scalar) or one octet row into two
// accumulators; kTwo == false means the second sum does not exist (no LDS,
// no work, no store). kTailRows (octet functors): how many partial rows per
// thread the ticket tail loads ahead of its adds — as many as fit in the
// registers the functor's streaming loop already takes, and no more, so the
// tail never costs the loop a wave of occupancy.

template <typename T, bool WANT_SQ>
struct ColSumElem {
  static constexpr bool kTwo = WANT_SQ;
  const T* x;
  struct Ch {};
  DEV_INLINE Ch channel(int) const { return {}; }
  DEV_INLINE void add(const Ch&, int64_t i, float& s, float& ss) const {
    const float v = ldf(&x[i]);
    s += v;
    if (WANT_SQ) ss += v * v;
  }
};

template <bool WANT_SQ>
struct ColSumRow8 {
  static constexpr bool kTwo = WANT_SQ;
  static constexpr int kTailRows = WANT_SQ ? 7 : 8;
  const bf16* x;
  struct Ch {};
  struct Row {
    bf16 x[8];
  };
  DEV_INLINE Ch channel(int) const { return {}; }
  DEV_INLINE void load(Row& v, int64_t i) const { ld8(v.x, x + i); }
  DEV_INLINE void add(const Ch&, const Row& v, float (&acc)[8],
                      float (&accsq)[8]) const {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float f = b2f(v.x[e]);
      acc[e] += f;
      if (WANT_SQ) accsq[e] += f * f;
    }
  }
};

// column sums of two fp32 [rows][C] partial matrices at once (the conv
// epilogue's sum and sumsq rows): s over a, ss over b
struct PartsElem {
  static constexpr bool kTwo = true;
  const float *a, *b;
  struct Ch {};
  DEV_INLINE Ch channel(int) const { return {}; }
  DEV_INLINE void add(const Ch&, int64_t i, float& s, float& ss) const {
    s += a[i];
    ss += b[i];
  }
};

// a1 = sum dpre (d_beta), a2 = sum dpre*xhat (d_gamma)
template <typename T, bool HAS_SKIP>
struct BnBwdElem {
  static constexpr bool kTwo = true;
  const T *dy, *x, *skip;
  BnParams p;
  int act;
  struct Ch {
    float mu, rsd, gm, bt;
  };
  DEV_INLINE Ch channel(int c) const {
    return {p.mean[c], p.rstd[c], p.gamma[c], p.beta[c]};
  }
  DEV_INLINE void add(const Ch& ch, int64_t i, float& a1, float& a2) const {
    const BnGrad g = bn_grad<HAS_SKIP>(
        ldf(&x[i]), ch.mu, ch.rsd, ch.gm, ch.bt,
        HAS_SKIP ? ldf(&skip[i]) : 0.f, ldf(&dy[i]), act);
    a1 += g.dpre;
    a2 += g.dpre * g.xh;
  }
};

template <bool HAS_SKIP>
struct BnBwdRow8 {
  static constexpr bool kTwo = true;
  static constexpr int kTailRows = 16;
  const bf16 *dy, *x, *skip;
  BnParams p;
  int act;
  using Ch = BnOct;
  struct Row {
    bf16 x[8], dy[8], skip[8];
  };
  DEV_INLINE Ch channel(int c0) const { return load_oct(p, c0); }
  DEV_INLINE void load(Row& v, int64_t i) const {
    ld8(v.x, x + i);
    ld8(v.dy, dy + i);
    if (HAS_SKIP) ld8(v.skip, skip + i);
  }
  DEV_INLINE void add(const Ch& ch, const Row& v, float (&a1)[8],
                      float (&a2)[8]) const {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const BnGrad g = bn_grad<HAS_SKIP>(
          b2f(v.x[e]), ch.mu[e], ch.rsd[e], ch.gm[e], ch.bt[e],
          HAS_SKIP ? b2f(v.skip[e]) : 0.f, b2f(v.dy[e]), act);
      a1[e] += g.dpre;
      a2[e] += g.dpre * g.xh;
    }
  }
};

// The separate OCTET kernels leave three contractions to the compiler,
// which fuses dy*act' into its consumers: sum dpre is fma(dy, act', a1), the
// sum with xhat is fma(xhat, round(dy*act'), a2), and the apply's
// dpre - s1/M is fma(dy, act', -s1/M). Inside the dual octet kernels the
// same source text contracts differently (the selects and the extra use of
// dpre are in the way), so there these three are written out. The scalar
// dual kernels keep the plain source text, which compiles to what the
// separate scalar kernels compute (tests/test_gpu_bn_dual.py holds both to
// torch.equal).
DEV_INLINE void dual_sums(bool second, const BnGrad& g, float dy, float sel,
                          float xh_s, float dsk, float& a1, float& a2) {
  a1 = __builtin_fmaf(second ? dsk : dy, second ? 1.f : sel, a1);
  a2 = __builtin_fmaf(second ? xh_s : g.xh, second ? dsk : g.dpre, a2);
}

// Dual backward sums. Virtual column cv < C: the main BN's sums of column cv
// (what BnBwd*<true> adds, with the skip recomputed); cv >= C: the skip
// BN's sums of column cv - C over dskip = round(dpre) (what BnBwd*<false>
// adds on the stored dskip, act Linear). A thread owns one virtual column
// (octet) and walks the rows its twin in the separate kernels walks.
template <typename T>
struct BnBwdDualElem {
  static constexpr bool kTwo = true;
  static constexpr int kPairs = 2;
  const T *dy, *x, *xs;
  BnParams p, ps;
  int act, C;
  struct Ch {
    float mu, rsd, gm, bt, mus, rsds, gms, bts;
    bool second;
  };
  DEV_INLINE Ch channel(int cv) const {
    const int c = cv % C;
    return {p.mean[c], p.rstd[c], p.gamma[c], p.beta[c], ps.mean[c],
            ps.rstd[c], ps.gamma[c], ps.beta[c], cv >= C};
  }
  DEV_INLINE void add(const Ch& ch, int64_t i, float& a1, float& a2) const {
    const float xsv = ldf(&xs[i]);
    const float dyv = ldf(&dy[i]);
    const float sk = bn_skip_elem<T>(xsv, ch.mus, ch.rsds, ch.gms, ch.bts);
    const BnGrad g = bn_grad<true>(ldf(&x[i]), ch.mu, ch.rsd, ch.gm, ch.bt,
                                   sk, dyv, act);
    const BnGrad gs = bn_grad<false>(xsv, ch.mus, ch.rsds, ch.gms, ch.bts,
                                     0.f, round_as<T>(g.dpre), ACT_LINEAR);
    const float d = ch.second ? gs.dpre : g.dpre;
    const float xh = ch.second ? gs.xh : g.xh;
    a1 += d;
    a2 += d * xh;
  }
};

struct BnBwdDualRow8 {
  static constexpr bool kTwo = true;
  static constexpr int kPairs = 2;
  static constexpr int kTailRows = 8;
  const bf16 *dy, *x, *xs;
  BnParams p, ps;
  int act, C;
  struct Ch {
    BnOct m, s;
    BnFold f;
    bool second;
  };
  struct Row {
    bf16 x[8], dy[8], xs[8];
  };
  DEV_INLINE Ch channel(int cv0) const {
    const int c0 = cv0 % C;
    return {load_oct(p, c0), load_oct(ps, c0), fold_oct(ps, c0), cv0 >= C};
  }
  DEV_INLINE void load(Row& v, int64_t i) const {
    ld8(v.x, x + i);
    ld8(v.dy, dy + i);
    ld8(v.xs, xs + i);
  }
  DEV_INLINE void add(const Ch& ch, const Row& v, float (&a1)[8],
                      float (&a2)[8]) const {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float xsv = b2f(v.xs[e]);
      const float dyv = b2f(v.dy[e]);
      const float sk = bn_skip_oct(xsv, ch.f.sc[e], ch.f.sh[e]);
      const BnGrad g = bn_grad<true>(b2f(v.x[e]), ch.m.mu[e], ch.m.rsd[e],
                                     ch.m.gm[e], ch.m.bt[e], sk, dyv, act);
      const BnGrad gs = bn_grad<false>(xsv, ch.s.mu[e], ch.s.rsd[e],
                                       ch.s.gm[e], ch.s.bt[e], 0.f,
                                       b2f(f2b(g.dpre)), ACT_LINEAR);
      dual_sums(ch.second, g, dyv, act_grad_by_sign(g.pre, act), gs.xh,
                gs.dpre, a1[e], a2[e]);
    }
  }
};

// ------------- deterministic finish of [chunks][C] partials, in-kernel -------
// The partial rows are summed in ONE fixed order whichever path runs:
//   chunks <= 8: out[c] = p[0][c] + p[1][c] + ...             (sequential)
//   chunks  > 8: 8 K-slices [K*s/8, K*(s+1)/8); per slice four sub-streams
//                k0+sub, +4, ... then sum4 -> stage[s][c]; out[c] = the
//                sequential sum of the 8 stage rows.
// The staged path does this with reduce_partials_kernel + reduce_final_kernel
// behind the reduce launch. The ticket path does it in the reduce launch's
// own tail: a block publishes its partial row and draws a ticket on its
// slice's counter; the block that draws the slice's last ticket reduces the
// slice and draws a ticket on the top counter; the last of those runs the
// final sum (and the BN finalize). Same reads, same adds, same order — the
// two paths are bitwise identical, and two dependent launches shorter.

// mean/rstd + running-stat update fused behind the final sum (mean != null)
struct BnFinalize {
  float* mean = nullptr;
  float* rstd = nullptr;
  float* run_mean = nullptr;
  float* run_var = nullptr;
  float Mf = 1.f, momentum = 0.1f, eps = 1e-5f;
};

// what the tail of a reduce launch needs; cnt == nullptr: no tail, the
// launch only writes partials (staged path)
struct BnTicket {
  int* cnt = nullptr;  // kTicketCounters lines of 128 B per blockIdx.x
  float *st1 = nullptr, *st2 = nullptr;  // [8][C] stage rows (chunks > 8)
  float *o1 = nullptr, *o2 = nullptr;    // [C] sums
  BnFinalize fin;
};

constexpr int kTicketSlices = 8;
constexpr int kTicketCounters = kTicketSlices + 1;  // 8 slices + top level

// out[c] = sequential sum of K rows of s1 (and s2), then the optional
// finalize: the whole per-channel work of the last stage. Up to 8 rows (all
// but the widest staged reduce) are loaded before the first add, so the
// block pays one memory round trip and not K dependent ones; the adds keep
// their order.
template <bool TWO>
DEV_INLINE void reduce_final_channel(const float* s1, const float* s2,
                                     float* o1, float* o2, int K, int C,
                                     int c, const BnFinalize& fin) {
  float a = 0.f, b = 0.f;
  if (K <= 8) {
    float va[8], vb[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      // always a valid row; 32-bit: the kernels' C is far below 2^28
      const unsigned i = (unsigned)min(k, K - 1) * (unsigned)C + c;
      va[k] = s1[i];
      if (TWO) vb[k] = s2[i];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (k < K) {
        a += va[k];
        if (TWO) b += vb[k];
      }
    }
  } else {
    for (int k = 0; k < K; ++k) a += s1[(int64_t)k * C + c];
    if (TWO) {
      for (int k = 0; k < K; ++k) b += s2[(int64_t)k * C + c];
    }
  }
  o1[c] = a;
  if (TWO) o2[c] = b;
  if (fin.mean) {
    const float mu = a / fin.Mf;
    float var = b / fin.Mf - mu * mu;
    var = fmaxf(var, 0.f);
    fin.mean[c] = mu;
    fin.rstd[c] = rsqrtf(var + fin.eps);
    if (fin.run_mean) {
      fin.run_mean[c] =
          (1.f - fin.momentum) * fin.run_mean[c] + fin.momentum * mu;
      const float ub = fin.Mf > 1.f ? var * fin.Mf / (fin.Mf - 1.f) : var;
      fin.run_var[c] =
          (1.f - fin.momentum) * fin.run_var[c] + fin.momentum * ub;
    }
  }
}

// A store another block of the same launch will read: write-through (sc1), so
// it needs no release fence behind it. A release fence writes the XCD's L2
// back once per block, and those serialise: the 1024-block stats reduce took
// 49 us with plain stores + a lane-0 release fence per block, 12 us with no
// tail at all (profiles/train_step_profile.md, "Single-launch BN reductions").
DEV_INLINE void st_publish(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Draws a ticket on *cnt once everything this block has st_publish-ed is
// out. True (in every thread) in the block that drew the last of n tickets;
// that block has acquired what the n-1 others published, and has put the
// counter back to zero for the next launch on the stream. Every storing
// wave drains its own stores ahead of the barrier; the ticket and the one
// acquire are lane 0's alone.
DEV_INLINE bool ticket_is_last(int* cnt, int n, int* flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const int t = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
    const bool last = t == n - 1;
    if (last) {
      __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    *flag = last ? 1 : 0;
  }
  __syncthreads();
  return *flag != 0;
}

// stage row of one K-slice for channels [c_lo, c_hi), 64 * V at a time:
// thread = (V adjacent channels, sub-stream); each accumulator sums exactly
// what its thread of reduce_partials_kernel sums, in that order. A slice of
// the flagship's 128 chunks is 64 KB per sum, read by this one block, which
// every other block of the launch is waiting for: U rows per thread are
// loaded (8 B per lane with V = 2) before the first add.
template <int V>
DEV_INLINE void ld_rowv(float (&v)[V], const float* p, unsigned off) {
  if constexpr (V == 2) {
    const float2 t = *reinterpret_cast<const float2*>(p + off);
    v[0] = t.x;
    v[1] = t.y;
  } else {
    v[0] = p[off];
  }
}

// NT: threads of the block; the slice is reduced by the first 256 (4
// sub-streams of 64), the others only keep the barriers.
template <bool TWO, int U, int V, int NT = 256>
DEV_INLINE void ticket_reduce_slice(const float* p1, const float* p2,
                                    float* o1, float* o2, int k0, int k1,
                                    int c_lo, int c_hi, int C, float* sh) {
  // 32-bit element offsets (chunks * C <= 1024 * 2048) on the uniform row
  // bases: one offset register serves both sums
  const int sub = threadIdx.x >> 6;
  const bool mine = NT == 256 || threadIdx.x < 256;
  for (int cb = c_lo; cb < c_hi; cb += 64 * V) {
    const int c = cb + (threadIdx.x & 63) * V;
    float a[V] = {}, b[V] = {};
    if (mine && c < c_hi) {
      // every round loads U rows before its first add, the last one too:
      // a row past the slice is loaded from row k instead and not added
      for (int k = k0 + sub; k < k1; k += 4 * U) {
        float va[U][V], vb[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int kk = k + 4 * u < k1 ? k + 4 * u : k;
          const unsigned off = (unsigned)kk * (unsigned)C + c;
          ld_rowv<V>(va[u], p1, off);
          if (TWO) ld_rowv<V>(vb[u], p2, off);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (k + 4 * u < k1) {
#pragma unroll
            for (int v = 0; v < V; ++v) {
              a[v] += va[u][v];
              if (TWO) b[v] += vb[u][v];
            }
          }
        }
      }
    }
    // sum4 tiles: [sum][v][256]
    if (mine) {
#pragma unroll
      for (int v = 0; v < V; ++v) {
        sh[v * 256 + threadIdx.x] = a[v];
        if (TWO) sh[(V + v) * 256 + threadIdx.x] = b[v];
      }
    }
    __syncthreads();
    if (sub == 0 && c < c_hi) {
#pragma unroll
      for (int v = 0; v < V; ++v) {
        st_publish(&o1[c + v], sum4(sh + v * 256));
        if (TWO) st_publish(&o2[c + v], sum4(sh + (V + v) * 256));
      }
    }
    __syncthreads();
  }
}

// Tail of a reduce launch, entered by every thread of every block after the
// block's partial row is stored. The block owns channels [c_lo, c_hi) of
// grid column blockIdx.x; sh is >= kTicketLds floats of the block's LDS
// that nobody reads any more.
// V = 2 needs c_lo, c_hi and C to be multiples of 128 and four sum4 tiles.
constexpr int kTicketLds = 2 * 256 + 1;  // two sum4 tiles + the "last" flag
constexpr int kTicketLdsWide = 4 * 256 + 1;
// counters sit one to a 128-B line: the tickets of a 1024-block launch on
// nine adjacent words serialise on that one line (about 17 ns each)
constexpr int kTicketStride = 32;

template <bool TWO, int U, bool WIDE, int NT = 256>
DEV_INLINE void ticket_finish(const BnTicket& t, const float* p1,
                              const float* p2, int c_lo, int c_hi, int C,
                              float* sh) {
  const int K = gridDim.y;
  int* cnt = t.cnt + blockIdx.x * (kTicketCounters * kTicketStride);
  int* flag = reinterpret_cast<int*>(sh + (WIDE ? 4 : 2) * 256);
  const float *f1 = p1, *f2 = p2;
  int fk = K;
  if (K > kTicketSlices) {
    int s = 0;  // the slice with k0 <= blockIdx.y < k1
    while ((K * (s + 1)) / kTicketSlices <= (int)blockIdx.y) ++s;
    const int k0 = (K * s) / kTicketSlices;
    const int k1 = (K * (s + 1)) / kTicketSlices;
    if (!ticket_is_last(cnt + s * kTicketStride, k1 - k0, flag)) return;
    float* o1 = t.st1 + (int64_t)s * C;
    float* o2 = t.st2 + (int64_t)s * C;
    if (WIDE && C % 128 == 0)
      ticket_reduce_slice<TWO, U, 2, NT>(p1, p2, o1, o2, k0, k1, c_lo, c_hi,
                                         C, sh);
    else
      ticket_reduce_slice<TWO, U, 1, NT>(p1, p2, o1, o2, k0, k1, c_lo, c_hi,
                                         C, sh);
    f1 = t.st1;
    f2 = t.st2;
    fk = kTicketSlices;
  }
  if (!ticket_is_last(cnt + kTicketSlices * kTicketStride, fk, flag)) return;
  if (NT != 256 && threadIdx.x >= 256) return;
  for (int c = c_lo + threadIdx.x; c < c_hi; c += 256)
    reduce_final_channel<TWO>(f1, f2, t.o1, t.o2, fk, C, c, t.fin);
}

// --------------------------- reduce skeletons -------------------------------
// Both: grid.y = row chunks; block y reduces rows [r0, r1) of every channel
// it owns and stores one partial row p1[y][C] (and p2[y][C]); with a ticket
// the launch also finishes the reduction (above).

// scalar, any C: block = 64 channels x 4 row sub-streams, grid (C/64, chunks).
// With a kPairs = 2 functor the columns are the 2C virtual ones (partial
// rows are 2C wide; the data rows stay C wide).
template <typename F>
__global__ void reduce_part_kernel(const F f, float* p1, float* p2,
                                   int64_t M, int Cd, const BnTicket tk) {
  constexpr int NP = reduce_pairs<F>::value;
  const int C = Cd * NP;  // columns of the partial rows
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int cd = NP == 1 ? c : c % Cd;  // column of the data rows
  const int sub = threadIdx.x >> 6;
  const bool live = c < C;
  const int64_t rows_per_chunk = (M + gridDim.y - 1) / gridDim.y;
  const int64_t r0 = blockIdx.y * rows_per_chunk;
  const int64_t r1 = min(M, r0 + rows_per_chunk);
  float a1 = 0.f, a2 = 0.f;
  if (live) {
    const typename F::Ch ch = f.channel(c);
    for (int64_t r = r0 + sub; r < r1; r += 4) f.add(ch, r * Cd + cd, a1, a2);
  }
  // one LDS object: the two sum4 tiles, and the ticket tail's flag word
  __shared__ float sh[kTicketLds];
  float* sh1 = sh;
  float* sh2 = sh + 256;
  sh1[threadIdx.x] = a1;
  if (F::kTwo) sh2[threadIdx.x] = a2;
  __syncthreads();
  if (sub == 0 && live) {
    st_publish(&p1[(int64_t)blockIdx.y * C + c], sum4(sh1));
    if (F::kTwo) st_publish(&p2[(int64_t)blockIdx.y * C + c], sum4(sh2));
  }
  if (tk.cnt)
    ticket_finish<F::kTwo, 8, false>(tk, p1, p2, blockIdx.x * 64,
                           min(C, (int)blockIdx.x * 64 + 64), C, sh);
}

// bf16 octets, C = 8*2^k: block = octs x streams threads, grid (1, chunks),
// LDS halving tree over the streams. UNROLL rows are loaded before any is
// consumed (independent 16-B loads in flight).
// A kPairs = 2 functor runs on 512 threads over the 2C virtual columns: the
// streams and their row walk are those of the 256-thread launch at C.
template <int UNROLL, typename F>
__global__ void reduce8_part_kernel(const F f, float* p1, float* p2,
                                    int64_t M, int Cd, const BnTicket tk) {
  constexpr int NP = reduce_pairs<F>::value;
  const int C = Cd * NP;  // columns of the partial rows
  const int octs = C >> 3;
  const int streams = blockDim.x / octs;
  const int oct = threadIdx.x % octs;
  const int rs = threadIdx.x / octs;
  const int c0 = oct * 8;
  const int cd0 = NP == 1 ? c0 : c0 % Cd;  // column of the data rows
  const int64_t rows_per_chunk = (M + gridDim.y - 1) / gridDim.y;
  const int64_t r0 = blockIdx.y * rows_per_chunk;
  const int64_t r1 = min(M, r0 + rows_per_chunk);
  const typename F::Ch ch = f.channel(c0);
  float a1[8] = {}, a2[8] = {};
  int64_t r = r0 + rs;
  for (; r + (UNROLL - 1) * (int64_t)streams < r1;
       r += UNROLL * (int64_t)streams) {
    typename F::Row v[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
      f.load(v[u], (r + u * (int64_t)streams) * Cd + cd0);
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) f.add(ch, v[u], a1, a2);
  }
  for (; r < r1; r += streams) {
    typename F::Row v;
    f.load(v, r * Cd + cd0);
    f.add(ch, v, a1, a2);
  }
  __shared__ float sh1[256 * NP][8];
  __shared__ float sh2[F::kTwo ? 256 * NP : 1][F::kTwo ? 8 : 1];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    sh1[threadIdx.x][e] = a1[e];
    if (F::kTwo) sh2[threadIdx.x][e] = a2[e];
  }
  __syncthreads();
  for (int off = streams >> 1; off > 0; off >>= 1) {
    if (rs < off) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        sh1[threadIdx.x][e] += sh1[threadIdx.x + off * octs][e];
        if (F::kTwo) sh2[threadIdx.x][e] += sh2[threadIdx.x + off * octs][e];
      }
    }
    __syncthreads();
  }
  if (rs == 0) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      st_publish(&p1[(int64_t)blockIdx.y * C + c0 + e], sh1[threadIdx.x][e]);
      if (F::kTwo)
        st_publish(&p2[(int64_t)blockIdx.y * C + c0 + e],
                   sh2[threadIdx.x][e]);
    }
  }
  // the tail borrows sh1 (2048 floats >= kTicketLdsWide): no further LDS
  // object
  static_assert(sizeof(sh1) >= kTicketLdsWide * sizeof(float), "tail LDS");
  if (tk.cnt)
    ticket_finish<F::kTwo, F::kTailRows, true, 256 * NP>(tk, p1, p2, 0, C,
                                                         C, &sh1[0][0]);
}

// ------------------------------ apply kernels -------------------------------
// Forward and backward-apply share their mapping (scalar: grid-stride with
// channel = i % C; octet: fixed octet per thread, rows gtid/octs + k*streams)
// but stay four separate kernels: written as functors on a shared shell they
// compile to different code. Pointers handed over inside a functor lose
// __restrict__, and the scalar loops then no longer unroll (about 950 -> 270
// instructions); the octet backward apply takes 90 instead of 79 VGPRs (one
// wave/SIMD less) even when the shell is called with __restrict__ pointers.

template <typename T, bool HAS_SKIP>
__global__ void bn_act_fwd_kernel(const T* __restrict__ x,
                                  const float* __restrict__ mean,
                                  const float* __restrict__ rstd,
                                  const float* __restrict__ gamma,
                                  const float* __restrict__ beta,
                                  const T* __restrict__ skip,
                                  T* __restrict__ y, int64_t n, int C,
                                  int act) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int c = i % C;
    const float xh = (ldf(&x[i]) - mean[c]) * rstd[c];
    float pre = xh * gamma[c] + beta[c];
    if (HAS_SKIP) pre += ldf(&skip[i]);
    stf(&y[i], apply_act(pre, act));
  }
}

// bf16 fast: fixed octet per thread -> per-channel params hoisted, here in
// the folded scale/shift form (NOT the same expression as the scalar one)
template <bool HAS_SKIP>
__global__ void bn_act_fwd8_kernel(const bf16* __restrict__ x,
                                   const float* __restrict__ mean,
                                   const float* __restrict__ rstd,
                                   const float* __restrict__ gamma,
                                   const float* __restrict__ beta,
                                   const bf16* __restrict__ skip,
                                   bf16* __restrict__ y, int64_t M, int C,
                                   int act) {
  const int octs = C >> 3;
  const int streams = (int)(((int64_t)blockDim.x * gridDim.y) / octs);
  const int64_t gtid = (int64_t)blockIdx.y * blockDim.x + threadIdx.x;
  const int oct = (int)(gtid % octs);
  const int64_t rs = gtid / octs;
  const int c0 = oct * 8;
  float sc[8], sh[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float g = gamma[c0 + e] * rstd[c0 + e];
    sc[e] = g;
    sh[e] = beta[c0 + e] - mean[c0 + e] * g;
  }
  for (int64_t r = rs; r < M; r += streams) {
    bf16 v[8], o[8], sk[8];
    ld8(v, &x[r * C + c0]);
    if (HAS_SKIP) ld8(sk, &skip[r * C + c0]);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float pre = b2f(v[e]) * sc[e] + sh[e];
      if (HAS_SKIP) pre += b2f(sk[e]);
      o[e] = f2b(apply_act(pre, act));
    }
    st8(&y[r * C + c0], o);
  }
}

// dx = gm*rsd*(dpre - s1/M - xhat*s2/M); dskip = dpre
template <typename T, bool HAS_SKIP>
__global__ void bn_act_bwd_apply_kernel(
    const T* __restrict__ dy, const T* __restrict__ x,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ s1, const float* __restrict__ s2,
    const T* __restrict__ skip, T* __restrict__ dskip,
    T* __restrict__ dx, int64_t n, int C, float Mf, int act) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int c = i % C;
    const float mu = mean[c], rs = rstd[c], gm = gamma[c];
    const BnGrad g = bn_grad<HAS_SKIP>(
        ldf(&x[i]), mu, rs, gm, beta[c],
        HAS_SKIP ? ldf(&skip[i]) : 0.f, ldf(&dy[i]), act);
    if (HAS_SKIP) stf(&dskip[i], g.dpre);
    stf(&dx[i], gm * rs * (g.dpre - s1[c] / Mf - g.xh * s2[c] / Mf));
  }
}

template <bool HAS_SKIP>
__global__ void bn_act_bwd_apply8_kernel(
    const bf16* __restrict__ dy, const bf16* __restrict__ x,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ s1, const float* __restrict__ s2,
    const bf16* __restrict__ skip, bf16* __restrict__ dskip,
    bf16* __restrict__ dx, int64_t M, int C, float Mf, int act) {
  const int octs = C >> 3;
  const int streams = (int)(((int64_t)blockDim.x * gridDim.y) / octs);
  const int64_t gtid = (int64_t)blockIdx.y * blockDim.x + threadIdx.x;
  const int oct = (int)(gtid % octs);
  const int64_t rs = gtid / octs;
  const int c0 = oct * 8;
  const float invM = 1.f / Mf;
  const BnOct ch = load_oct({mean, rstd, gamma, beta}, c0);
  float t1[8], t2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    t1[e] = s1[c0 + e] * invM;
    t2[e] = s2[c0 + e] * invM;
  }
  for (int64_t r = rs; r < M; r += streams) {
    bf16 vx[8], vdy[8], o[8], vsk[8], osk[8];
    ld8(vx, &x[r * C + c0]);
    ld8(vdy, &dy[r * C + c0]);
    if (HAS_SKIP) ld8(vsk, &skip[r * C + c0]);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const BnGrad g = bn_grad<HAS_SKIP>(
          b2f(vx[e]), ch.mu[e], ch.rsd[e], ch.gm[e], ch.bt[e],
          HAS_SKIP ? b2f(vsk[e]) : 0.f, b2f(vdy[e]), act);
      if (HAS_SKIP) osk[e] = f2b(g.dpre);
      o[e] = f2b(ch.gm[e] * ch.rsd[e] * (g.dpre - t1[e] - g.xh * t2[e]));
    }
    if (HAS_SKIP) st8(&dskip[r * C + c0], osk);
    st8(&dx[r * C + c0], o);
  }
}

// ---- dual apply kernels: the element-wise code of the two kernels they
// replace, back to back, with the tensor between them kept in a register

template <typename T>
__global__ void bn_act_fwd_dual_kernel(const T* __restrict__ x,
                                       const T* __restrict__ xs,
                                       const BnParams p, const BnParams ps,
                                       T* __restrict__ y, int64_t n, int C,
                                       int act) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int c = i % C;
    const float sk = bn_skip_elem<T>(ldf(&xs[i]), ps.mean[c], ps.rstd[c],
                                     ps.gamma[c], ps.beta[c]);
    const float xh = (ldf(&x[i]) - p.mean[c]) * p.rstd[c];
    float pre = xh * p.gamma[c] + p.beta[c];
    pre += sk;
    stf(&y[i], apply_act(pre, act));
  }
}

__global__ void bn_act_fwd_dual8_kernel(const bf16* __restrict__ x,
                                        const bf16* __restrict__ xs,
                                        const BnParams p, const BnParams ps,
                                        bf16* __restrict__ y, int64_t M,
                                        int C, int act) {
  const int octs = C >> 3;
  const int streams = (int)(((int64_t)blockDim.x * gridDim.y) / octs);
  const int64_t gtid = (int64_t)blockIdx.y * blockDim.x + threadIdx.x;
  const int oct = (int)(gtid % octs);
  const int64_t rs = gtid / octs;
  const int c0 = oct * 8;
  const BnFold f = fold_oct(p, c0);
  const BnFold fs = fold_oct(ps, c0);
  for (int64_t r = rs; r < M; r += streams) {
    bf16 v[8], vs[8], o[8];
    ld8(v, &x[r * C + c0]);
    ld8(vs, &xs[r * C + c0]);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float sk = bn_skip_oct(b2f(vs[e]), fs.sc[e], fs.sh[e]);
      float pre = b2f(v[e]) * f.sc[e] + f.sh[e];
      pre += sk;
      o[e] = f2b(apply_act(pre, act));
    }
    st8(&y[r * C + c0], o);
  }
}

// s1/s2: [2C] sums, the skip BN's in the second half
template <typename T>
__global__ void bn_act_bwd_dual_apply_kernel(
    const T* __restrict__ dy, const T* __restrict__ x,
    const T* __restrict__ xs, const BnParams p, const BnParams ps,
    const float* __restrict__ s1, const float* __restrict__ s2,
    T* __restrict__ dx, T* __restrict__ dxs, int64_t n, int C, float Mf,
    int act) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int c = i % C;
    const float mu = p.mean[c], rs = p.rstd[c], gm = p.gamma[c];
    const float mus = ps.mean[c], rss = ps.rstd[c], gms = ps.gamma[c];
    const float xsv = ldf(&xs[i]);
    const float sk = bn_skip_elem<T>(xsv, mus, rss, gms, ps.beta[c]);
    const float dyv = ldf(&dy[i]);
    const BnGrad g = bn_grad<true>(ldf(&x[i]), mu, rs, gm, p.beta[c], sk,
                                   dyv, act);
    stf(&dx[i], gm * rs * (g.dpre - s1[c] / Mf - g.xh * s2[c] / Mf));
    const BnGrad gs = bn_grad<false>(xsv, mus, rss, gms, ps.beta[c], 0.f,
                                     round_as<T>(g.dpre), ACT_LINEAR);
    stf(&dxs[i],
        gms * rss * (gs.dpre - s1[C + c] / Mf - gs.xh * s2[C + c] / Mf));
  }
}

__global__ __launch_bounds__(256) void bn_act_bwd_dual_apply8_kernel(
    const bf16* __restrict__ dy, const bf16* __restrict__ x,
    const bf16* __restrict__ xs, const BnParams p, const BnParams ps,
    const float* __restrict__ s1, const float* __restrict__ s2,
    bf16* __restrict__ dx, bf16* __restrict__ dxs, int64_t M, int C,
    float Mf, int act) {
  const int octs = C >> 3;
  const int streams = (int)(((int64_t)blockDim.x * gridDim.y) / octs);
  const int64_t gtid = (int64_t)blockIdx.y * blockDim.x + threadIdx.x;
  const int oct = (int)(gtid % octs);
  const int64_t rs = gtid / octs;
  const int c0 = oct * 8;
  const float invM = 1.f / Mf;
  const BnOct ch = load_oct(p, c0);
  const BnOct cs = load_oct(ps, c0);
  const BnFold fs = fold_oct(ps, c0);
  float t1[8], t2[8], u1[8], u2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    t1[e] = s1[c0 + e] * invM;
    t2[e] = s2[c0 + e] * invM;
    u1[e] = s1[C + c0 + e] * invM;
    u2[e] = s2[C + c0 + e] * invM;
  }
  for (int64_t r = rs; r < M; r += streams) {
    bf16 vx[8], vdy[8], vxs[8], o[8], os[8];
    ld8(vx, &x[r * C + c0]);
    ld8(vdy, &dy[r * C + c0]);
    ld8(vxs, &xs[r * C + c0]);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float xsv = b2f(vxs[e]);
      const float sk = bn_skip_oct(xsv, fs.sc[e], fs.sh[e]);
      const float dyv = b2f(vdy[e]);
      const BnGrad g = bn_grad<true>(b2f(vx[e]), ch.mu[e], ch.rsd[e],
                                     ch.gm[e], ch.bt[e], sk, dyv, act);
      const float d1 =
          __builtin_fmaf(dyv, act_grad_by_sign(g.pre, act), -t1[e]);
      o[e] = f2b(ch.gm[e] * ch.rsd[e] * __builtin_fmaf(-g.xh, t2[e], d1));
      const BnGrad gs = bn_grad<false>(xsv, cs.mu[e], cs.rsd[e], cs.gm[e],
                                       cs.bt[e], 0.f, b2f(f2b(g.dpre)),
                                       ACT_LINEAR);
      os[e] = f2b(cs.gm[e] * cs.rsd[e] *
                  __builtin_fmaf(-gs.xh, u2[e], gs.dpre - u1[e]));
    }
    st8(&dx[r * C + c0], o);
    st8(&dxs[r * C + c0], os);
  }
}

// ------------- staged finish of [chunks][C] partials: two launches -----------

// stage1[ks][c] = sum of the ks-th K-slice of p[k][c] (and stage2/p2).
// block = 64 channels x 4 k-substreams (a K=256 serial loop in one tiny
// block was 44 us — latency-bound). grid (C/64, KSPLIT); a tiny second
// kernel sums the KSPLIT staged rows in FIXED order (the earlier
// same-address atomicAdd finish made BN statistics — and so the whole
// training trajectory — vary with fp add order).
__global__ void reduce_partials_kernel(const float* __restrict__ p1,
                                       const float* __restrict__ p2,
                                       float* __restrict__ o1,
                                       float* __restrict__ o2,
                                       int K, int C) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int sub = threadIdx.x >> 6;
  const int k0 = (K * blockIdx.y) / gridDim.y;
  const int k1 = (K * (blockIdx.y + 1)) / gridDim.y;
  float a = 0.f, b = 0.f;
  if (c < C) {
    for (int k = k0 + sub; k < k1; k += 4) {
      a += p1[(int64_t)k * C + c];
      if (p2) b += p2[(int64_t)k * C + c];
    }
  }
  __shared__ float sha[256], shb[256];
  sha[threadIdx.x] = a;
  shb[threadIdx.x] = b;
  __syncthreads();
  if (sub == 0 && c < C) {
    o1[(int64_t)blockIdx.y * C + c] = sum4(sha);
    if (p2) o2[(int64_t)blockIdx.y * C + c] = sum4(shb);
  }
}

// Optionally fuses the BN finalize (mean/rstd + running-stat update) so
// bn_stats is one kernel shorter (fin_mean != nullptr selects it).
__global__ void reduce_final_kernel(const float* __restrict__ s1,
                                    const float* __restrict__ s2,
                                    float* __restrict__ o1,
                                    float* __restrict__ o2, int K, int C,
                                    float* __restrict__ fin_mean = nullptr,
                                    float* __restrict__ fin_rstd = nullptr,
                                    float* __restrict__ run_mean = nullptr,
                                    float* __restrict__ run_var = nullptr,
                                    float Mf = 1.f, float momentum = 0.1f,
                                    float eps = 1e-5f) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  BnFinalize fin;
  fin.mean = fin_mean;
  fin.rstd = fin_rstd;
  fin.run_mean = run_mean;
  fin.run_var = run_var;
  fin.Mf = Mf;
  fin.momentum = momentum;
  fin.eps = eps;
  if (o2) reduce_final_channel<true>(s1, s2, o1, o2, K, C, c, fin);
  else reduce_final_channel<false>(s1, s2, o1, o2, K, C, c, fin);
}

// --------------------------------- host -------------------------------------

static BnFinalize make_finalize(torch::Tensor& mean, torch::Tensor& rstd,
                                c10::optional<torch::Tensor>& running_mean,
                                c10::optional<torch::Tensor>& running_var,
                                int64_t M, double momentum, double eps) {
  BnFinalize fin;
  fin.mean = mean.data_ptr<float>();
  fin.rstd = rstd.data_ptr<float>();
  if (running_mean.has_value()) {
    TORCH_CHECK(running_mean->scalar_type() == at::kFloat);
    fin.run_mean = running_mean->data_ptr<float>();
    fin.run_var = running_var->data_ptr<float>();
  }
  fin.Mf = (float)M;
  fin.momentum = (float)momentum;
  fin.eps = (float)eps;
  return fin;
}

// staged two-kernel deterministic reduction of [chunks][C] partials
static void run_reduce_partials(const float* p1, const float* p2,
                                float* o1, float* o2, int chunks, int C,
                                const torch::TensorOptions& opt,
                                hipStream_t s,
                                const BnFinalize& fin = BnFinalize{}) {
  auto finish = [&](const float* s1, const float* s2, int K) {
    hipLaunchKernelGGL(reduce_final_kernel, dim3(cdiv(C, 256)), dim3(256),
        0, s, s1, s2, o1, o2, K, C, fin.mean, fin.rstd, fin.run_mean,
        fin.run_var, fin.Mf, fin.momentum, fin.eps);
  };
  if (chunks <= 8) {
    // stage 1 would be a pure copy (each y-block owns exactly one row):
    // reduce the partials directly in fixed order
    finish(p1, p2, chunks);
    return;
  }
  // ks sets BOTH stage-1 parallelism and the single-block stage-2 loop
  // length: ks=8 is right for the common <=1024-chunk reduces (scaling
  // it with chunks made stage 2 latency-bound — measured 5 -> 16 us);
  // only the opt-in conv-epilogue stats path (up to 4096 rows) needs a
  // wider stage 1
  int ks = 8;
  if (chunks > 1024) ks = std::min(256, chunks / 16);
  auto st = torch::empty({(int64_t)2 * ks * C}, opt);
  float* s1 = st.data_ptr<float>();
  float* s2 = p2 ? s1 + (int64_t)ks * C : nullptr;
  hipLaunchKernelGGL(reduce_partials_kernel, dim3(cdiv(C, 64), ks),
      dim3(256), 0, s, p1, p2, s1, s2, chunks, C);
  finish(s1, s2, ks);
}

// ---- ticket counters: one zeroed int32 page per (device, stream) ----------
// Every counter is put back to zero by the block that draws its last ticket,
// so consecutive launches on a stream share one page with no memset node
// between them; launches on different streams may overlap and get different
// pages. Pages are cut from a per-device pool that is allocated and zeroed
// on the first eager (non-capturing) call; handing a page of an existing
// pool to a new stream touches no memory, so it is legal during stream
// capture — a hipGraph captured after an eager warm-up gets the ticket path
// on its own capture stream. With no pool yet (or none left) during a
// capture, that call takes the staged path. The kernels of one captured
// graph share the capture stream's page: replays of graphs captured on the
// same stream must not overlap each other (they never do here: one stream
// replays them in order).

// >= kTicketCounters * kTicketStride * grid.x: 14 grid columns, C <= 896 on
// the scalar skeleton (wider ones stay staged)
constexpr int kTicketPageInts = 4096;
constexpr int kTicketPoolPages = 32;

static bool bn_stream_capturing(hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &st) != hipSuccess) {
    (void)hipGetLastError();
    return true;  // be conservative: allocate nothing
  }
  return st != hipStreamCaptureStatusNone;
}

// nullptr: take the staged path
static int* ticket_counters(const torch::Tensor& like, hipStream_t s,
                            int grid_x) {
  const char* e = getenv("RTHD_BN_STAGED");
  if (e && e[0] == '1' && e[1] == '\0') return nullptr;
  if ((int64_t)grid_x * kTicketCounters * kTicketStride > kTicketPageInts)
    return nullptr;
  struct Pool {
    std::vector<torch::Tensor> slabs;
    int used = 0;  // pages handed out of slabs.back()
  };
  static std::mutex mu;
  static std::map<int, Pool> pools;
  static std::map<std::pair<int, hipStream_t>, int*> pages;
  const int dev = like.device().index();
  std::lock_guard<std::mutex> lk(mu);
  auto it = pages.find({dev, s});
  if (it != pages.end()) return it->second;
  Pool& pool = pools[dev];
  if (pool.slabs.empty() || pool.used == kTicketPoolPages) {
    if (bn_stream_capturing(s)) return nullptr;
    pool.slabs.push_back(torch::zeros(
        {(int64_t)kTicketPoolPages * kTicketPageInts},
        like.options().dtype(at::kInt)));
    pool.used = 0;
    // the zero fill ran on s; any other stream may be handed a page later
    if (hipStreamSynchronize(s) != hipSuccess) {
      (void)hipGetLastError();
      pool.slabs.pop_back();
      pool.used = kTicketPoolPages;
      return nullptr;
    }
  }
  int* page = pool.slabs.back().data_ptr<int>() +
              (int64_t)pool.used++ * kTicketPageInts;
  pages.emplace(std::make_pair(dev, s), page);
  return page;
}

// The finish of one reduce launch: a ticket for the launch to finish itself
// (tk.cnt set), or, staged, the two finish launches behind it.
struct BnFinish {
  BnTicket tk;
  torch::Tensor stage;  // keeps tk.st1/st2 alive

  BnFinish(const torch::Tensor& like, int grid_x, int chunks, int C,
           float* o1, float* o2, const torch::TensorOptions& opt,
           hipStream_t s, const BnFinalize& fin = BnFinalize{}) {
    tk.cnt = ticket_counters(like, s, grid_x);
    if (!tk.cnt) return;
    if (chunks > kTicketSlices) {
      stage = torch::empty({(int64_t)2 * kTicketSlices * C}, opt);
      tk.st1 = stage.data_ptr<float>();
      tk.st2 = tk.st1 + (int64_t)kTicketSlices * C;
    }
    tk.o1 = o1;
    tk.o2 = o2;
    tk.fin = fin;
  }
};

// runtime bool / dtype -> compile-time argument of a generic lambda
template <typename Fn>
static void with_bool(bool b, Fn&& fn) {
  if (b) fn(std::true_type{});
  else fn(std::false_type{});
}

template <typename T>
struct TypeTag {
  using type = T;
};

template <typename Fn>
static void with_dtype(const torch::Tensor& t, Fn&& fn) {
  if (t.scalar_type() == at::kBFloat16) {
    fn(TypeTag<bf16>{});
  } else {
    TORCH_CHECK(t.scalar_type() == at::kFloat, "bf16/f32 only");
    fn(TypeTag<float>{});
  }
}

// typed data pointer; nullptr for an undefined (absent) tensor
template <typename T>
static T* ptr(const torch::Tensor& t) {
  return t.defined() ? reinterpret_cast<T*>(t.data_ptr()) : nullptr;
}

static BnParams bn_params(const torch::Tensor& mean, const torch::Tensor& rstd,
                          const torch::Tensor& gm, const torch::Tensor& bt) {
  return {mean.data_ptr<float>(), rstd.data_ptr<float>(),
          gm.data_ptr<float>(), bt.data_ptr<float>()};
}

// one launch site per reduce skeleton
template <typename F>
static void launch_reduce(const F& f, float* p1, float* p2, int chunks,
                          int64_t M, int C, hipStream_t s,
                          const BnTicket& tk) {
  constexpr int NP = reduce_pairs<F>::value;
  hipLaunchKernelGGL((reduce_part_kernel<F>), dim3(cdiv(NP * C, 64), chunks),
      dim3(256), 0, s, f, p1, p2, M, C, tk);
}

template <int UNROLL, typename F>
static void launch_reduce8(const F& f, float* p1, float* p2, int chunks,
                           int64_t M, int C, hipStream_t s,
                           const BnTicket& tk) {
  constexpr int NP = reduce_pairs<F>::value;
  hipLaunchKernelGGL((reduce8_part_kernel<UNROLL, F>), dim3(1, chunks),
      dim3(256 * NP), 0, s, f, p1, p2, M, C, tk);
}

// grid of the octet apply kernels: (1, nb) blocks of 256
static int rows8_blocks(int64_t M, int C) {
  return (int)std::min<int64_t>(cdiv(M * (C / 8), 256), 2048);
}

static void run_colsum(const torch::Tensor& xc, torch::Tensor& sum,
                       torch::Tensor* sumsq, int64_t M, int C,
                       hipStream_t s,
                       const BnFinalize& fin = BnFinalize{}) {
  const int chunks = pick_chunks(M, C);
  auto p1 = torch::empty({chunks, C}, sum.options());
  torch::Tensor p2;
  if (sumsq) p2 = torch::empty({chunks, C}, sum.options());
  float* p1p = p1.data_ptr<float>();
  float* p2p = ptr<float>(p2);
  float* o1p = sum.data_ptr<float>();
  float* o2p = sumsq ? sumsq->data_ptr<float>() : nullptr;
  const bool fast8 = fast8_ok(xc, C);
  const BnFinish done(xc, fast8 ? 1 : (int)cdiv(C, 64), chunks, C, o1p, o2p,
                      sum.options(), s, fin);
  with_bool(sumsq != nullptr, [&](auto want_sq) {
    constexpr bool SQ = decltype(want_sq)::value;
    if (fast8) {
      // 4x unrolled: one 16-B load per loop iteration leaves only ~4 MB in
      // flight across the chip (< the ~6 MB needed to cover HBM latency at
      // 8 TB/s); four independent loads per iteration saturate the bus.
      launch_reduce8<4>(ColSumRow8<SQ>{ptr<const bf16>(xc)}, p1p, p2p,
                        chunks, M, C, s, done.tk);
    } else {
      with_dtype(xc, [&](auto tag) {
        using T = typename decltype(tag)::type;
        launch_reduce(ColSumElem<T, SQ>{ptr<const T>(xc)}, p1p, p2p, chunks,
                      M, C, s, done.tk);
      });
    }
  });
  if (!done.tk.cnt)
    run_reduce_partials(p1p, p2p, o1p, o2p, chunks, C, sum.options(), s,
                        fin);
}

std::vector<torch::Tensor> bn_stats(torch::Tensor x,
                                    c10::optional<torch::Tensor> running_mean,
                                    c10::optional<torch::Tensor> running_var,
                                    double momentum, double eps) {
  auto xc = x.contiguous(at::MemoryFormat::ChannelsLast);
  const int C = xc.size(1);
  const int64_t M = xc.numel() / C;
  // fully overwritten by the final sum (no zero-init kernels)
  auto sum = torch::empty({C}, xc.options().dtype(at::kFloat));
  auto sumsq = torch::empty({C}, xc.options().dtype(at::kFloat));
  auto mean = torch::empty({C}, xc.options().dtype(at::kFloat));
  auto rstd = torch::empty({C}, xc.options().dtype(at::kFloat));
  auto s = at::cuda::getCurrentCUDAStream();
  run_colsum(xc, sum, &sumsq, M, C, s,  // finalize fused in
             make_finalize(mean, rstd, running_mean, running_var, M,
                           momentum, eps));
  HIP_CHECK_LAST();
  return {mean, rstd};
}

// finalize mean/rstd from the conv-epilogue-fused column partials
// (conv_fwd_stats): p1/p2 are [rows, C] sum / sumsq rows, reduced in fixed
// order. M = number of pixels (B*Ho*Wo). The partials are reduced like any
// other [rows][C] matrix: one launch of the scalar reduce skeleton over
// chunks of 32 rows that finishes itself through the ticket tail and writes
// mean, rstd and the running statistics there (make_finalize); without a
// ticket page (first call inside a capture) the staged launches follow.
std::vector<torch::Tensor> bn_stats_from_parts(
    torch::Tensor p1, torch::Tensor p2,
    c10::optional<torch::Tensor> running_mean,
    c10::optional<torch::Tensor> running_var,
    double momentum, double eps, int64_t M) {
  TORCH_CHECK(p1.dim() == 2 && p1.sizes() == p2.sizes() &&
              p1.scalar_type() == at::kFloat &&
              p2.scalar_type() == at::kFloat,
              "bn_stats_from_parts: bad partials");
  auto a = p1.contiguous();
  auto b = p2.contiguous();
  const int64_t rows = a.size(0);
  const int C = a.size(1);
  auto opt = a.options();
  auto sum = torch::empty({C}, opt);
  auto sumsq = torch::empty({C}, opt);
  auto mean = torch::empty({C}, opt);
  auto rstd = torch::empty({C}, opt);
  auto s = at::cuda::getCurrentCUDAStream();
  const BnFinalize fin = make_finalize(mean, rstd, running_mean, running_var,
                                       M, momentum, eps);
  // 8 rows per thread: short enough to stay latency-light, long enough that
  // the flagship's 8192-row layers finish in 256 chunk rows
  const int chunks = (int)std::min<int64_t>(1024, cdiv(rows, (int64_t)32));
  auto q1 = torch::empty({chunks, C}, opt);
  auto q2 = torch::empty({chunks, C}, opt);
  const BnFinish done(a, (int)cdiv(C, 64), chunks, C, sum.data_ptr<float>(),
                      sumsq.data_ptr<float>(), opt, s, fin);
  launch_reduce(PartsElem{a.data_ptr<float>(), b.data_ptr<float>()},
                q1.data_ptr<float>(), q2.data_ptr<float>(), chunks, rows, C,
                s, done.tk);
  if (!done.tk.cnt)
    run_reduce_partials(q1.data_ptr<float>(), q2.data_ptr<float>(),
                        sum.data_ptr<float>(), sumsq.data_ptr<float>(),
                        chunks, C, opt, s, fin);
  HIP_CHECK_LAST();
  return {mean, rstd};
}

torch::Tensor bn_act_fwd(torch::Tensor x, torch::Tensor mean,
                         torch::Tensor rstd, torch::Tensor gamma,
                         torch::Tensor beta, int64_t act,
                         c10::optional<torch::Tensor> skip) {
  auto xc = x.contiguous(at::MemoryFormat::ChannelsLast);
  const int C = xc.size(1);
  const int64_t n = xc.numel();
  const int64_t M = n / C;
  auto y = torch::empty_like(xc);
  auto gm = gamma.to(at::kFloat).contiguous();
  auto bt = beta.to(at::kFloat).contiguous();
  auto s = at::cuda::getCurrentCUDAStream();
  const bool has_skip = skip.has_value();
  torch::Tensor sk;
  if (has_skip)
    sk = skip->to(xc.scalar_type()).contiguous(at::MemoryFormat::ChannelsLast);
  const BnParams p = bn_params(mean, rstd, gm, bt);
  const bool fast8 = fast8_ok(xc, C);
  with_bool(has_skip, [&](auto hs) {
    constexpr bool HS = decltype(hs)::value;
    if (fast8) {
      hipLaunchKernelGGL((bn_act_fwd8_kernel<HS>), dim3(1, rows8_blocks(M, C)),
          dim3(256), 0, s, ptr<const bf16>(xc), p.mean, p.rstd, p.gamma,
          p.beta, ptr<const bf16>(sk), ptr<bf16>(y), M, C, (int)act);
    } else {
      with_dtype(xc, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL((bn_act_fwd_kernel<T, HS>), dim3(ew_grid(n, 256)),
            dim3(256), 0, s, ptr<const T>(xc), p.mean, p.rstd, p.gamma,
            p.beta, ptr<const T>(sk), ptr<T>(y), n, C, (int)act);
      });
    }
  });
  HIP_CHECK_LAST();
  return y;
}

std::vector<torch::Tensor> bn_act_bwd(torch::Tensor dy, torch::Tensor x,
                                      torch::Tensor mean, torch::Tensor rstd,
                                      torch::Tensor gamma, torch::Tensor beta,
                                      int64_t act,
                                      c10::optional<torch::Tensor> skip) {
  auto xc = x.contiguous(at::MemoryFormat::ChannelsLast);
  auto dyc = dy.to(xc.scalar_type()).contiguous(at::MemoryFormat::ChannelsLast);
  const int C = xc.size(1);
  const int64_t n = xc.numel();
  const int64_t M = n / C;
  auto s1 = torch::empty({C}, xc.options().dtype(at::kFloat));
  auto s2 = torch::empty({C}, xc.options().dtype(at::kFloat));
  auto dx = torch::empty_like(xc);
  auto gm = gamma.to(at::kFloat).contiguous();
  auto bt = beta.to(at::kFloat).contiguous();
  auto s = at::cuda::getCurrentCUDAStream();
  const bool has_skip = skip.has_value();
  torch::Tensor sk, dsk;
  if (has_skip) {
    sk = skip->to(xc.scalar_type()).contiguous(at::MemoryFormat::ChannelsLast);
    dsk = torch::empty_like(xc);
  }

  const int chunks = pick_chunks(M, C);
  auto p1 = torch::empty({chunks, C}, s1.options());
  auto p2 = torch::empty({chunks, C}, s1.options());
  float* p1p = p1.data_ptr<float>();
  float* p2p = p2.data_ptr<float>();
  float* s1p = s1.data_ptr<float>();
  float* s2p = s2.data_ptr<float>();
  const BnParams p = bn_params(mean, rstd, gm, bt);
  const bool fast8 = fast8_ok(xc, C);
  const BnFinish done(xc, fast8 ? 1 : (int)cdiv(C, 64), chunks, C, s1p, s2p,
                      s1.options(), s);
  with_bool(has_skip, [&](auto hs) {
    constexpr bool HS = decltype(hs)::value;
    // reduce -> fixed-order finish -> apply, on one mapping
    auto run = [&](auto tag, auto octet) {
      using T = typename decltype(tag)::type;
      constexpr bool OCT = decltype(octet)::value;
      const T* pdy = ptr<const T>(dyc);
      const T* px = ptr<const T>(xc);
      const T* ps = ptr<const T>(sk);
      if constexpr (OCT) {
        // 2x unrolled (2-3 loads/iter already): 4-6 independent loads in
        // flight (4x was measured SLOWER: 71 -> 98 us — register pressure)
        launch_reduce8<2>(BnBwdRow8<HS>{pdy, px, ps, p, (int)act}, p1p, p2p,
                          chunks, M, C, s, done.tk);
      } else {
        launch_reduce(BnBwdElem<T, HS>{pdy, px, ps, p, (int)act}, p1p, p2p,
                      chunks, M, C, s, done.tk);
      }
      if (!done.tk.cnt)
        run_reduce_partials(p1p, p2p, s1p, s2p, chunks, C, s1.options(), s);
      if constexpr (OCT) {
        hipLaunchKernelGGL((bn_act_bwd_apply8_kernel<HS>),
            dim3(1, rows8_blocks(M, C)), dim3(256), 0, s, pdy, px, p.mean,
            p.rstd, p.gamma, p.beta, s1p, s2p, ps, ptr<T>(dsk), ptr<T>(dx),
            M, C, (float)M, (int)act);
      } else {
        hipLaunchKernelGGL((bn_act_bwd_apply_kernel<T, HS>),
            dim3(ew_grid(n, 256)), dim3(256), 0, s, pdy, px, p.mean, p.rstd,
            p.gamma, p.beta, s1p, s2p, ps, ptr<T>(dsk), ptr<T>(dx), n, C,
            (float)M, (int)act);
      }
    };
    if (fast8) {
      run(TypeTag<bf16>{}, std::true_type{});
    } else {
      with_dtype(xc, [&](auto tag) { run(tag, std::false_type{}); });
    }
  });
  HIP_CHECK_LAST();
  // dgamma = s2, dbeta = s1; dskip (= dpre) last when skip given
  if (has_skip) return {dx, s2, s1, dsk};
  return {dx, s2, s1};
}

// ---- dual forms: main BN on x, skip BN (Linear) on xs; see the file header

static void check_dual(const torch::Tensor& xc, const torch::Tensor& xsc) {
  TORCH_CHECK(xc.sizes() == xsc.sizes() &&
              xc.scalar_type() == xsc.scalar_type(),
              "bn dual: x and xs must agree in shape and dtype");
}

torch::Tensor bn_act_fwd_dual(torch::Tensor x, torch::Tensor mean,
                              torch::Tensor rstd, torch::Tensor gamma,
                              torch::Tensor beta, torch::Tensor xs,
                              torch::Tensor mean_s, torch::Tensor rstd_s,
                              torch::Tensor gamma_s, torch::Tensor beta_s,
                              int64_t act) {
  auto xc = x.contiguous(at::MemoryFormat::ChannelsLast);
  auto xsc = xs.contiguous(at::MemoryFormat::ChannelsLast);
  check_dual(xc, xsc);
  const int C = xc.size(1);
  const int64_t n = xc.numel();
  const int64_t M = n / C;
  auto y = torch::empty_like(xc);
  auto gm = gamma.to(at::kFloat).contiguous();
  auto bt = beta.to(at::kFloat).contiguous();
  auto gms = gamma_s.to(at::kFloat).contiguous();
  auto bts = beta_s.to(at::kFloat).contiguous();
  auto s = at::cuda::getCurrentCUDAStream();
  const BnParams p = bn_params(mean, rstd, gm, bt);
  const BnParams ps = bn_params(mean_s, rstd_s, gms, bts);
  if (fast8_ok(xc, C)) {
    hipLaunchKernelGGL(bn_act_fwd_dual8_kernel, dim3(1, rows8_blocks(M, C)),
        dim3(256), 0, s, ptr<const bf16>(xc), ptr<const bf16>(xsc), p, ps,
        ptr<bf16>(y), M, C, (int)act);
  } else {
    with_dtype(xc, [&](auto tag) {
      using T = typename decltype(tag)::type;
      hipLaunchKernelGGL((bn_act_fwd_dual_kernel<T>), dim3(ew_grid(n, 256)),
          dim3(256), 0, s, ptr<const T>(xc), ptr<const T>(xsc), p, ps,
          ptr<T>(y), n, C, (int)act);
    });
  }
  HIP_CHECK_LAST();
  return y;
}

// {dx, dgamma, dbeta, dxs, dgamma_s, dbeta_s}
std::vector<torch::Tensor> bn_act_bwd_dual(
    torch::Tensor dy, torch::Tensor x, torch::Tensor mean,
    torch::Tensor rstd, torch::Tensor gamma, torch::Tensor beta,
    torch::Tensor xs, torch::Tensor mean_s, torch::Tensor rstd_s,
    torch::Tensor gamma_s, torch::Tensor beta_s, int64_t act) {
  auto xc = x.contiguous(at::MemoryFormat::ChannelsLast);
  auto xsc = xs.contiguous(at::MemoryFormat::ChannelsLast);
  check_dual(xc, xsc);
  auto dyc = dy.to(xc.scalar_type()).contiguous(at::MemoryFormat::ChannelsLast);
  const int C = xc.size(1);
  const int64_t n = xc.numel();
  const int64_t M = n / C;
  const auto fopt = xc.options().dtype(at::kFloat);
  // [2C]: the main BN's sums, then the skip BN's
  auto s1 = torch::empty({2 * C}, fopt);
  auto s2 = torch::empty({2 * C}, fopt);
  auto dx = torch::empty_like(xc);
  auto dxs = torch::empty_like(xc);
  auto gm = gamma.to(at::kFloat).contiguous();
  auto bt = beta.to(at::kFloat).contiguous();
  auto gms = gamma_s.to(at::kFloat).contiguous();
  auto bts = beta_s.to(at::kFloat).contiguous();
  auto s = at::cuda::getCurrentCUDAStream();
  const BnParams p = bn_params(mean, rstd, gm, bt);
  const BnParams ps = bn_params(mean_s, rstd_s, gms, bts);

  // the chunking of the separate kernels: M and C, not 2C
  const int chunks = pick_chunks(M, C);
  auto p1 = torch::empty({chunks, 2 * C}, fopt);
  auto p2 = torch::empty({chunks, 2 * C}, fopt);
  float* p1p = p1.data_ptr<float>();
  float* p2p = p2.data_ptr<float>();
  float* s1p = s1.data_ptr<float>();
  float* s2p = s2.data_ptr<float>();
  const bool fast8 = fast8_ok(xc, C);
  const BnFinish done(xc, fast8 ? 1 : (int)cdiv(2 * C, 64), chunks, 2 * C,
                      s1p, s2p, fopt, s);
  auto run = [&](auto tag, auto octet) {
    using T = typename decltype(tag)::type;
    constexpr bool OCT = decltype(octet)::value;
    const T* pdy = ptr<const T>(dyc);
    const T* px = ptr<const T>(xc);
    const T* pxs = ptr<const T>(xsc);
    if constexpr (OCT) {
      // not unrolled: two rows of three loads in flight put the functor's
      // 64 hoisted parameters over the 128 registers of a 512-thread block
      // (the adds keep their order whatever the unroll)
      launch_reduce8<1>(BnBwdDualRow8{pdy, px, pxs, p, ps, (int)act, C}, p1p,
                        p2p, chunks, M, C, s, done.tk);
    } else {
      launch_reduce(BnBwdDualElem<T>{pdy, px, pxs, p, ps, (int)act, C}, p1p,
                    p2p, chunks, M, C, s, done.tk);
    }
    if (!done.tk.cnt)
      run_reduce_partials(p1p, p2p, s1p, s2p, chunks, 2 * C, fopt, s);
    if constexpr (OCT) {
      hipLaunchKernelGGL(bn_act_bwd_dual_apply8_kernel,
          dim3(1, rows8_blocks(M, C)), dim3(256), 0, s, pdy, px, pxs, p, ps,
          s1p, s2p, ptr<T>(dx), ptr<T>(dxs), M, C, (float)M, (int)act);
    } else {
      hipLaunchKernelGGL((bn_act_bwd_dual_apply_kernel<T>),
          dim3(ew_grid(n, 256)), dim3(256), 0, s, pdy, px, pxs, p, ps, s1p,
          s2p, ptr<T>(dx), ptr<T>(dxs), n, C, (float)M, (int)act);
    }
  };
  if (fast8) {
    run(TypeTag<bf16>{}, std::true_type{});
  } else {
    with_dtype(xc, [&](auto tag) { run(tag, std::false_type{}); });
  }
  HIP_CHECK_LAST();
  return {dx, s2.narrow(0, 0, C), s1.narrow(0, 0, C), dxs,
          s2.narrow(0, C, C), s1.narrow(0, C, C)};
}

// plain column sum (conv dbias): sum over rows of (M, C)
torch::Tensor col_sum(torch::Tensor x) {
  auto xc = x.contiguous(at::MemoryFormat::ChannelsLast);
  const int C = xc.size(1);
  const int64_t M = xc.numel() / C;
  auto sum = torch::empty({C}, xc.options().dtype(at::kFloat));
  auto s = at::cuda::getCurrentCUDAStream();
  run_colsum(xc, sum, nullptr, M, C, s);
  HIP_CHECK_LAST();
  return sum;
}

}  // namespace rthd
