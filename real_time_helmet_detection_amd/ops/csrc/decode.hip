// Fused CenterNet decode: 3x3(pool_size) peak mask + top-k + offset/size
// gather + box construction.
//
// Replaces the reference decode chain (transform.py:73-110: maxpool ->
// eq-mask -> mul -> flat topk -> div/mod -> 4 gathers -> arithmetic).
// Round-1 ran the whole thing as ONE workgroup per image: at batch 1 that
// is one 256-thread block scanning C*H*W pixels twice on a 256-CU chip —
// 495 us, 33% of b1 inference (profiles). Round 2 splits it:
//
//   k1 decode_scan   GRID-WIDE peak scan: every surviving 3x3-local-max
//                    appends (score, idx) to a per-image peak buffer
//                    (<= PCAP) and bumps a per-image 1024-bin histogram.
//   k2 decode_thr    one thread per image: pick the threshold bin so
//                    >= K candidates survive.
//   k3 decode_emit   one workgroup per image: filter the peak buffer by
//                    the threshold, bitonic-sort (desc, idx-stable) in
//                    LDS and emit exactly K (box, class, score) rows.
//                    If the peak buffer overflowed (plateau-heavy
//                    degenerate inputs), fall back to re-scanning the
//                    image in-block (the round-1 path, correctness
//                    preserved).
//
// The atomic append order is nondeterministic but the sort's total order
// (score desc, idx asc — matching torch.topk's stable order) makes the
// OUTPUT deterministic and identical to the single-block version.
//
// Two front ends share k2, k3 and the candidate plumbing:
//
//   decode_fwd     post-sigmoid fp32 maps (hm, off, wh) in; k1 reads every
//                  pixel's neighbourhood from global memory.
//   decode_logits  the raw (Bt,S,C+4,H,W) network output in, bf16 or fp32:
//                  upcast, sigmoid and (flip test) the merge with the
//                  mirrored half happen at the load. k1 is tiled: a block
//                  stages one tile + halo of one (image, stack, class)
//                  plane into LDS as merged fp32 probabilities — each
//                  evaluated once — and tests peaks from LDS. k3 gathers
//                  offset/size from the logits at the K winners only, so
//                  no merged map is ever written to memory.
//
// k3 reads its maps through a source struct (MapSrc / LogitSrc): prob()
// is the heatmap value at a pixel, geom() the offset/size pair there.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include "common.h"

namespace rthd {

constexpr int NBINS = 1024;
constexpr int CAP = 2048;   // sorted-candidate capacity (pow2 for bitonic)
constexpr int PCAP = 8192;  // raw peak-buffer capacity per image

// decode_logits scan tile: 256 threads, one pixel each, halo <= RMAX
constexpr int TW = 32;
constexpr int TH = 8;
constexpr int RMAX = 3;     // pool_size 3, 5, 7

struct Cand {
  float score;
  int idx;
};

// post-sigmoid fp32 maps: hm (N,C,H,W), off / wh (N,2,H,W)
struct MapSrc {
  const float* hm;
  const float* off;
  const float* wh;
  int C, H, W;

  DEV_INLINE float prob(int img, int c, int y, int x) const {
    return hm[((int64_t)img * C + c) * H * W + y * W + x];
  }
  DEV_INLINE void geom(int img, int y, int x, float& xo, float& yo,
                       float& xs, float& ys) const {
    const int64_t HWl = (int64_t)H * W;
    const int rem = y * W + x;
    const float* off_b = off + (int64_t)img * 2 * HWl;
    const float* wh_b = wh + (int64_t)img * 2 * HWl;
    xo = off_b[rem];
    yo = off_b[HWl + rem];
    xs = wh_b[rem];
    ys = wh_b[HWl + rem];
  }
};

// full-precision expf: scores are user-visible and compared to the CPU
// oracle at the decode tolerances
DEV_INLINE float sigmoidf_(float z) { return 1.f / (1.f + expf(-z)); }

// raw logits (Bt,S,C+4,H,W); image img = b*S + s. Under FLIP item B+b is
// the network's output for the mirrored image b: heatmap and size are the
// mean of the plain value at x and the mirrored value at W-1-x (the same
// cache lines read backwards, so the load stays coalesced); offsets come
// from the plain half only.
template <typename T, bool FLIP>
struct LogitSrc {
  const T* out;
  int B, S, C, H, W;
  bool squash_geom;  // normalized coordinates: sigmoid on offset and size

  DEV_INLINE const T* plane(int img, int ch, bool mirrored) const {
    const int b = img / S, s = img % S;
    const int64_t bb = mirrored ? b + B : b;
    return out + ((bb * S + s) * (C + 4) + ch) * ((int64_t)H * W);
  }
  DEV_INLINE float merged(int img, int ch, int y, int x, bool squash) const {
    float v = ldf(plane(img, ch, false) + y * W + x);
    if (squash) v = sigmoidf_(v);
    if (FLIP) {
      float m = ldf(plane(img, ch, true) + y * W + (W - 1 - x));
      if (squash) m = sigmoidf_(m);
      v = 0.5f * (v + m);
    }
    return v;
  }
  DEV_INLINE float prob(int img, int c, int y, int x) const {
    return merged(img, c, y, x, true);
  }
  DEV_INLINE void geom(int img, int y, int x, float& xo, float& yo,
                       float& xs, float& ys) const {
    xo = ldf(plane(img, C, false) + y * W + x);
    yo = ldf(plane(img, C + 1, false) + y * W + x);
    if (squash_geom) {
      xo = sigmoidf_(xo);
      yo = sigmoidf_(yo);
    }
    xs = merged(img, C + 2, y, x, squash_geom);
    ys = merged(img, C + 3, y, x, squash_geom);
  }
};

template <class Src>
DEV_INLINE bool is_peak_at(const Src& src, int img, float v,
                           int c, int y, int x, int R) {
  for (int dy = -R; dy <= R; ++dy) {
    const int ys = y + dy;
    if (ys < 0 || ys >= src.H) continue;
    for (int dx = -R; dx <= R; ++dx) {
      const int xs = x + dx;
      if (xs < 0 || xs >= src.W) continue;
      if (src.prob(img, c, ys, xs) > v) return false;
    }
  }
  return true;
}

DEV_INLINE int score_bin(float v) {
  int bin = (int)(v * NBINS);
  return bin < 0 ? 0 : (bin >= NBINS ? NBINS - 1 : bin);
}

// a surviving local max joins image img's histogram and peak buffer
DEV_INLINE void append_peak(Cand* __restrict__ peaks, int* __restrict__ pcount,
                            int* __restrict__ hist, int img, float v, int j) {
  atomicAdd(&hist[(int64_t)img * NBINS + score_bin(v)], 1);
  const int slot = atomicAdd(&pcount[img], 1);
  if (slot < PCAP) {
    peaks[(int64_t)img * PCAP + slot].score = v;
    peaks[(int64_t)img * PCAP + slot].idx = j;
  }
}

__global__ void decode_scan_kernel(
    MapSrc src,                        // hm (B, C, H, W) post-sigmoid
    Cand* __restrict__ peaks,          // (B, PCAP)
    int* __restrict__ pcount,          // (B)
    int* __restrict__ hist,            // (B, NBINS)
    int B, int R) {
  const int H = src.H, W = src.W;
  const int n = src.C * H * W;
  const int64_t total = (int64_t)B * n;
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    const int b = (int)(i / n);
    const int j = (int)(i % n);
    const float v = src.hm[i];
    if (v <= 0.f) continue;
    const int c = j / (H * W);
    const int rem = j % (H * W);
    const int y = rem / W, x = rem % W;
    if (!is_peak_at(src, b, v, c, y, x, R)) continue;
    append_peak(peaks, pcount, hist, b, v, j);
  }
}

// Tiled scan over raw logits. grid (tiles, C, images); the block stages its
// TH x TW tile plus an R-wide halo into LDS as merged probabilities, then
// every thread tests its own pixel against the LDS window. Pixels outside
// the map are staged as -1, below every probability, so tile tails and map
// borders need no special case in the test; no global address is formed
// for them.
template <typename T, bool FLIP>
__global__ __launch_bounds__(TW * TH) void decode_logits_scan_kernel(
    LogitSrc<T, FLIP> src, Cand* __restrict__ peaks,
    int* __restrict__ pcount, int* __restrict__ hist, int R) {
  __shared__ float tile[TH + 2 * RMAX][TW + 2 * RMAX];
  const int H = src.H, W = src.W;
  const int img = blockIdx.z, c = blockIdx.y;
  const int tiles_x = (W + TW - 1) / TW;
  const int x0 = (blockIdx.x % tiles_x) * TW;
  const int y0 = (blockIdx.x / tiles_x) * TH;
  const int tw = TW + 2 * R, th = TH + 2 * R;
  for (int i = threadIdx.x; i < tw * th; i += TW * TH) {
    const int ly = i / tw, lx = i % tw;
    const int gy = y0 - R + ly, gx = x0 - R + lx;
    float v = -1.f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = src.prob(img, c, gy, gx);
    tile[ly][lx] = v;
  }
  __syncthreads();
  const int tx = threadIdx.x % TW, ty = threadIdx.x / TW;
  const int x = x0 + tx, y = y0 + ty;
  if (x >= W || y >= H) return;
  const float v = tile[ty + R][tx + R];
  if (v <= 0.f) return;
  for (int dy = 0; dy <= 2 * R; ++dy)
    for (int dx = 0; dx <= 2 * R; ++dx)
      if (tile[ty + dy][tx + dx] > v) return;
  append_peak(peaks, pcount, hist, img, v, (c * H + y) * W + x);
}

// one block per image: the histogram is staged into LDS with coalesced
// vector loads first (a single thread walking 1024 bins straight from
// HBM measured 70 us — one full memory latency per bin)
__global__ void decode_thr_kernel(const int* __restrict__ hist,
                                  int* __restrict__ thr, int B, int K) {
  const int b = blockIdx.x;
  // 16-B alignment for the int4 staging loads (guide G17: misaligned
  // b128 LDS accesses replay at 64 cycles each)
  __shared__ __attribute__((aligned(16))) int h[NBINS];
  const int* hg = hist + (int64_t)b * NBINS;
  for (int i = threadIdx.x * 4; i < NBINS; i += blockDim.x * 4)
    *reinterpret_cast<int4*>(&h[i]) =
        *reinterpret_cast<const int4*>(&hg[i]);
  __syncthreads();
  if (threadIdx.x == 0) {
    int suffix = 0, t = 0;
    for (int bin = NBINS - 1; bin >= 0; --bin) {
      suffix += h[bin];
      if (suffix >= K) { t = bin; break; }
    }
    // the lowest bin that still leaves K candidates: the emit stage
    // takes any number of them, CAP at a time
    thr[b] = t;
  }
}

// bitonic sort of cands[0..ncand) desc (ties: lower idx first — torch.topk
// stable order), padded in place to a pow2 region; ends on a barrier
DEV_INLINE void sort_cands(Cand* cands, int ncand) {
  int P = 64;
  while (P < ncand) P <<= 1;
  for (int i = threadIdx.x + ncand; i < P; i += blockDim.x) {
    cands[i].score = -1.f;
    cands[i].idx = 0x7fffffff;
  }
  __syncthreads();
  for (int k2 = 2; k2 <= P; k2 <<= 1) {
    for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
      for (int i = threadIdx.x; i < P / 2; i += blockDim.x) {
        const int a = (i / j2) * (j2 * 2) + (i % j2);
        const int bgt = a ^ j2;
        if (bgt > a) {
          const bool dirDesc = ((a & k2) == 0);
          Cand ca = cands[a], cb = cands[bgt];
          const bool a_lt_b = (ca.score < cb.score) ||
              (ca.score == cb.score && ca.idx > cb.idx);
          if (dirDesc == a_lt_b) {
            cands[a] = cb;
            cands[bgt] = ca;
          }
        }
      }
      __syncthreads();
    }
  }
}

// Candidates arrive in chunks of source entries into a 2*CAP LDS array; a
// chunk is as long as the array has room for if every entry passed. Up to
// 2*CAP source entries are one chunk and one sort. Beyond that (plateaus:
// thousands of peaks sharing the threshold bin) an array more than half
// full is sorted and cut to its best K <= CAP before the next chunk — the
// top K of a set under a total order do not depend on the order of
// arrival, so the output stays deterministic.
template <class Src>
__global__ void decode_emit_kernel(
    Src src, const Cand* __restrict__ peaks,
    const int* __restrict__ pcount, const int* __restrict__ thr,
    float* __restrict__ boxes, int64_t* __restrict__ clss,
    float* __restrict__ scores, int K, int R, float sf, int normalized) {
  const int b = blockIdx.x;
  const int H = src.H, W = src.W;
  const int n = src.C * H * W;
  const int thr_bin = thr[b];
  const int npk = pcount[b];

  __shared__ Cand cands[2 * CAP];
  __shared__ int counter;
  if (threadIdx.x == 0) counter = 0;
  __syncthreads();

  // common path: filter the pre-collected peaks; overflow (degenerate
  // plateau-heavy input): re-scan the image in-block
  const bool rescan = npk > PCAP;
  const int nsrc = rescan ? n : npk;
  const Cand* pb = peaks + (int64_t)b * PCAP;
  for (int base = 0, len = 0; base < nsrc; base += len) {
    int cur = counter;
    __syncthreads();
    if (cur > CAP) {
      sort_cands(cands, cur);
      cur = cur < K ? cur : K;
      if (threadIdx.x == 0) counter = cur;
      __syncthreads();
    }
    // cur <= CAP: room for at least CAP more
    len = nsrc - base < 2 * CAP - cur ? nsrc - base : 2 * CAP - cur;
    for (int j = base + threadIdx.x; j < base + len; j += blockDim.x) {
      Cand cd;
      if (!rescan) {
        cd = pb[j];
        if (score_bin(cd.score) < thr_bin) continue;
      } else {
        const int c = j / (H * W);
        const int rem = j % (H * W);
        const float v = src.prob(b, c, rem / W, rem % W);
        if (v <= 0.f || score_bin(v) < thr_bin) continue;
        if (!is_peak_at(src, b, v, c, rem / W, rem % W, R)) continue;
        cd.score = v;
        cd.idx = j;
      }
      const int slot = atomicAdd(&counter, 1);
      if (slot < 2 * CAP) cands[slot] = cd;
    }
    __syncthreads();
  }

  const int ncand = counter < 2 * CAP ? counter : 2 * CAP;
  sort_cands(cands, ncand);

  for (int i = threadIdx.x; i < K; i += blockDim.x) {
    float sc = 0.f;
    int idx = 0;
    if (i < ncand && cands[i].score > 0.f) {
      sc = cands[i].score;
      idx = cands[i].idx;
    }
    const int c = idx / (H * W);
    const int rem = idx % (H * W);
    const int y = rem / W, x = rem % W;
    float xo, yo, xs, ys;
    src.geom(b, y, x, xo, yo, xs, ys);
    if (normalized) {
      xo *= sf;
      yo *= sf;
      xs *= (float)W;
      ys *= (float)H;
    }
    const float xc = (float)x + xo, yc = (float)y + yo;
    float* bo = boxes + ((int64_t)b * K + i) * 4;
    bo[0] = (xc - xs * 0.5f) * sf;
    bo[1] = (yc - ys * 0.5f) * sf;
    bo[2] = (xc + xs * 0.5f) * sf;
    bo[3] = (yc + ys * 0.5f) * sf;
    clss[(int64_t)b * K + i] = c;
    scores[(int64_t)b * K + i] = sc;
  }
}

// outputs + scratch of one decode over N images; the counters and the
// histogram are zeroed on-stream (capture-legal)
struct DecodeBuffers {
  torch::Tensor boxes, clss, scores, peaks, ws;
  Cand* peakp;
  int* pcount;
  int* thr;
  int* hist;

  DecodeBuffers(int64_t N, int64_t topk, const torch::TensorOptions& fopt) {
    boxes = torch::empty({N, topk, 4}, fopt);
    clss = torch::empty({N, topk}, fopt.dtype(at::kLong));
    scores = torch::empty({N, topk}, fopt);
    peaks = torch::empty({N * PCAP * 2}, fopt);
    // pcount[N] + thr[N] + hist[N][NBINS], zeroed in one fill
    ws = torch::zeros({N * (NBINS + 2)}, fopt.dtype(at::kInt));
    peakp = reinterpret_cast<Cand*>(peaks.data_ptr<float>());
    pcount = ws.data_ptr<int>();
    thr = pcount + N;
    hist = thr + N;
  }
};

// k2 + k3 behind either scan
template <class Src>
static void launch_thr_emit(const Src& src, DecodeBuffers& d, int N,
                            int64_t topk, int R, int64_t scale_factor,
                            bool normalized, hipStream_t s) {
  hipLaunchKernelGGL(decode_thr_kernel, dim3(N), dim3(256), 0, s,
      d.hist, d.thr, N, (int)topk);
  hipLaunchKernelGGL((decode_emit_kernel<Src>), dim3(N), dim3(256), 0, s,
      src, d.peakp, d.pcount, d.thr, d.boxes.data_ptr<float>(),
      d.clss.data_ptr<int64_t>(), d.scores.data_ptr<float>(), (int)topk, R,
      (float)scale_factor, normalized ? 1 : 0);
  HIP_CHECK_LAST();
}

std::vector<torch::Tensor> decode_fwd(torch::Tensor hm, torch::Tensor off,
                                      torch::Tensor wh, int64_t scale_factor,
                                      int64_t topk, int64_t pool_size,
                                      bool normalized) {
  auto hm_ = hm.to(at::kFloat).contiguous();
  auto off_ = off.to(at::kFloat).contiguous();
  auto wh_ = wh.to(at::kFloat).contiguous();
  const int B = hm_.size(0), C = hm_.size(1);
  const int H = hm_.size(2), W = hm_.size(3);
  TORCH_CHECK(topk <= CAP, "decode: topk > capacity");

  DecodeBuffers d(B, topk, hm_.options());
  const MapSrc src{hm_.data_ptr<float>(), off_.data_ptr<float>(),
                   wh_.data_ptr<float>(), C, H, W};
  const int R = (int)(pool_size / 2);

  auto s = at::cuda::getCurrentCUDAStream();
  const int64_t total = (int64_t)B * C * H * W;
  hipLaunchKernelGGL(decode_scan_kernel, dim3(ew_grid(total, 256)),
      dim3(256), 0, s, src, d.peakp, d.pcount, d.hist, B, R);
  launch_thr_emit(src, d, B, topk, R, scale_factor, normalized, s);
  return {d.boxes, d.clss, d.scores};
}

template <typename T, bool FLIP>
static void decode_logits_launch(const torch::Tensor& out_, DecodeBuffers& d,
                                 int B, int S, int C, int H, int W,
                                 int64_t scale_factor, int64_t topk, int R,
                                 bool normalized) {
  const LogitSrc<T, FLIP> src{reinterpret_cast<const T*>(out_.data_ptr()),
                              B, S, C, H, W, normalized};
  const int N = B * S;
  const int tiles = (int)(cdiv(W, TW) * cdiv(H, TH));
  auto s = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL((decode_logits_scan_kernel<T, FLIP>),
      dim3(tiles, C, N), dim3(TW * TH), 0, s, src, d.peakp, d.pcount,
      d.hist, R);
  launch_thr_emit(src, d, N, topk, R, scale_factor, normalized, s);
}

std::vector<torch::Tensor> decode_logits(torch::Tensor out,
                                         int64_t scale_factor, int64_t topk,
                                         int64_t pool_size, bool normalized,
                                         bool flip) {
  TORCH_CHECK(out.dim() == 5 && out.size(2) > 4,
              "decode_logits: out must be (B,S,C+4,H,W)");
  const bool is_bf16 = out.scalar_type() == at::kBFloat16;
  TORCH_CHECK(is_bf16 || out.scalar_type() == at::kFloat,
              "decode_logits: out must be bf16 or f32");
  auto out_ = out.contiguous();
  const int64_t Bt = out_.size(0);
  TORCH_CHECK(!flip || Bt % 2 == 0,
              "decode_logits: flip needs an even batch (plain half then "
              "mirrored half), got ", Bt);
  const int B = (int)(flip ? Bt / 2 : Bt), S = out_.size(1);
  const int C = out_.size(2) - 4;
  const int H = out_.size(3), W = out_.size(4);
  const int R = (int)(pool_size / 2);
  TORCH_CHECK(topk >= 1 && topk <= CAP, "decode_logits: topk outside 1..",
              CAP);
  TORCH_CHECK(pool_size >= 1 && R <= RMAX, "decode_logits: pool_size > ",
              2 * RMAX + 1);
  TORCH_CHECK(H >= 1 && W >= 1 && (int64_t)C * H * W < (1ll << 31),
              "decode_logits: map size");
  const int64_t N = (int64_t)B * S;
  TORCH_CHECK(N <= 65535 && C <= 65535, "decode_logits: grid too large");

  DecodeBuffers d(N, topk, out_.options().dtype(at::kFloat));
  if (N == 0) return {d.boxes, d.clss, d.scores};

#define RTHD_DECODE_LOGITS(T, F)                                          \
  decode_logits_launch<T, F>(out_, d, B, S, C, H, W, scale_factor, topk,  \
                             R, normalized)
  if (is_bf16) {
    if (flip) RTHD_DECODE_LOGITS(bf16, true);
    else      RTHD_DECODE_LOGITS(bf16, false);
  } else {
    if (flip) RTHD_DECODE_LOGITS(float, true);
    else      RTHD_DECODE_LOGITS(float, false);
  }
#undef RTHD_DECODE_LOGITS
  return {d.boxes, d.clss, d.scores};
}

}  // namespace rthd
