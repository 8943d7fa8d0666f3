// Gaussian soft-NMS, one wave per image.
//
// Replaces the eager loop of ops/eager.py soft_nms (reference
// evaluate.py:184-243) on GPU tensors. Semantics, per image, in fp32:
// candidates with score >= conf take part; round 1 selects the highest
// score unconditionally (ties -> lowest original index); after each
// selection every remaining score is multiplied by exp(-(iou^2)/sigma) and
// a candidate whose score is <= score_th is dropped for good; later rounds
// select the maximum of what remains until nothing remains.
//
// Design: SINGLE WAVE, barrier-free rounds. The algorithm is a serial chain
// of up to L rounds (L = live candidates), each an argmax followed by an
// elementwise decay, so latency per round is what matters. A typical image
// has L = 100-250, i.e. 2-4 candidates per lane: a 256-thread block would
// leave three of four waves with nothing to do and pay two s_barrier
// round trips plus an LDS exchange of the per-wave maxima every round,
// where one wave needs none of that. Per round the wave
//   1. takes the winner (wave-uniform, from the previous reduction) and
//      reads its box from LDS at a uniform address (broadcast),
//   2. makes ONE pass over its lane-strided candidates (p = lane + 64k,
//      conflict-free LDS rows) that fuses the decay by this winner with the
//      argmax for the next round,
//   3. reduces a 64-bit key (order-preserving score bits << 32 | ~position)
//      with six DPP steps (row_shr 1/2/4/8, row_bcast15, row_bcast31) and a
//      readlane of lane 63 — no LDS traffic, no ds_bpermute latency.
// The key's low half makes a score tie go to the lowest compacted position,
// and the up-front compaction keeps original order, so that is the lowest
// original index (torch.argmax's first occurrence). Candidates below conf
// are compacted away first (ballot + prefix popcount), so rounds scale
// with L, not N. Dead candidates hold NaN in the live-score row.
// No atomics, no host sync, no allocation that depends on data.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <limits>

#include "nms_common.h"

namespace rthd {

// order-preserving float <-> uint map (0 is reached only by a NaN, which
// never passes the conf filter, so key 0 means "nothing live")
DEV_INLINE unsigned f2ord(float f) {
  const unsigned u = __float_as_uint(f);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
DEV_INLINE float ord2f(unsigned k) {
  return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k);
}

template <int CTRL, int ROW_MASK>
DEV_INLINE unsigned long long dpp_max_step(unsigned long long v) {
  const int lo = (int)(unsigned)v;
  const int hi = (int)(unsigned)(v >> 32);
  // lanes without a valid source (or in a masked-off row) get `old` = own
  const int olo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf,
                                              false);
  const int ohi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf,
                                              false);
  const unsigned long long o =
      ((unsigned long long)(unsigned)ohi << 32) | (unsigned)olo;
  return o > v ? o : v;
}

// max over the 64 lanes, wave-uniform result. All 64 lanes must be active.
DEV_INLINE unsigned long long wave_max_u64(unsigned long long v) {
  v = dpp_max_step<0x111, 0xf>(v);  // row_shr:1
  v = dpp_max_step<0x112, 0xf>(v);  // row_shr:2
  v = dpp_max_step<0x114, 0xf>(v);  // row_shr:4
  v = dpp_max_step<0x118, 0xf>(v);  // row_shr:8  -> lane 15 of each row
  v = dpp_max_step<0x142, 0xa>(v);  // row_bcast15 into rows 1 and 3
  v = dpp_max_step<0x143, 0xc>(v);  // row_bcast31 into rows 2 and 3
  const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)v, 63);
  const unsigned hi = __builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
  return ((unsigned long long)hi << 32) | lo;
}

DEV_INLINE unsigned long long snms_key(float s, int p) {
  return ((unsigned long long)f2ord(s) << 32) | (0xffffffffu - (unsigned)p);
}

// grid.x = image, block = one wave. PACK: the packed emit of nms_pack
// (nms_common.h) replaces the three output arrays, which are then null.
template <bool PACK>
__global__ __launch_bounds__(64) void soft_nms_kernel(
    const float* __restrict__ boxes,   // (B,N,4)
    const float* __restrict__ scores,  // (B,N)
    int* __restrict__ out_idx,         // (B,N) zero-filled
    float* __restrict__ out_scores,    // (B,N) zero-filled
    int* __restrict__ out_count,       // (B,)
    int N, float sigma, float score_th, float conf, NmsPack pk) {
  __shared__ float sx1[NMS_CAP], sy1[NMS_CAP], sx2[NMS_CAP], sy2[NMS_CAP];
  __shared__ float ss[NMS_CAP];  // live score, NaN once selected or dropped
  __shared__ int sorig[NMS_CAP];

  const int bimg = blockIdx.x;
  const int lane = threadIdx.x;
  const float4* b4 =
      reinterpret_cast<const float4*>(boxes + (int64_t)bimg * N * 4);
  scores += (int64_t)bimg * N;
  if (!PACK) {
    out_idx += (int64_t)bimg * N;
    out_scores += (int64_t)bimg * N;
  }

  // ---- compact the candidates with score >= conf, order preserved ----
  int L = 0;
#pragma unroll 4
  for (int i0 = 0; i0 < N; i0 += 64) {
    const int i = i0 + lane;
    const bool in = i < N;
    const float s = in ? scores[i] : 0.f;
    const float4 bb = in ? b4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const bool keep = in && (s >= conf);
    const unsigned long long m = __ballot(keep);
    if (keep) {
      const int p = L + __popcll(m & ((1ull << lane) - 1ull));
      sx1[p] = bb.x;
      sy1[p] = bb.y;
      sx2[p] = bb.z;
      sy2[p] = bb.w;
      ss[p] = s;
      sorig[p] = i;
    }
    L += __popcll(m);
  }
  __syncthreads();  // one wave: orders the LDS image, costs nothing

  // ---- round 1: plain argmax over everything that passed conf ----
  unsigned long long best = 0ull;
  for (int p = lane; p < L; p += 64) {
    const unsigned long long k = snms_key(ss[p], p);
    best = k > best ? k : best;
  }
  best = wave_max_u64(best);

  const float nan = __uint_as_float(0x7fc00000u);
  int cnt = 0;
  while (best != 0ull) {
    const int pstar = (int)(0xffffffffu - (unsigned)best);
    const float wscore = ord2f((unsigned)(best >> 32));
    const float wx1 = sx1[pstar], wy1 = sy1[pstar];
    const float wx2 = sx2[pstar], wy2 = sy2[pstar];
    const float warea = box_area(wx1, wy1, wx2, wy2);
    if (lane == 0) {
      if (PACK) {
        nms_pack_record(pk, bimg, N, cnt, sorig[pstar], wx1, wy1, wx2, wy2,
                        wscore);
      } else {
        out_idx[cnt] = sorig[pstar];
        out_scores[cnt] = wscore;
      }
    }
    ++cnt;

    // decay by this winner fused with the argmax for the next round
    best = 0ull;
    for (int p = lane; p < L; p += 64) {
      float s = ss[p];
      if (s != s) continue;  // already selected or dropped
      if (p != pstar) {
        const float x1 = sx1[p], y1 = sy1[p], x2 = sx2[p], y2 = sy2[p];
        const float iou = box_iou(wx1, wy1, wx2, wy2, warea, x1, y1, x2, y2);
        s = s * expf(-(iou * iou) / sigma);
        if (s > score_th) {
          const unsigned long long k = snms_key(s, p);
          best = k > best ? k : best;
        } else {
          s = nan;
        }
      } else {
        s = nan;
      }
      ss[p] = s;
    }
    best = wave_max_u64(best);
  }
  if (PACK) {
    // header and zero tail: with the records above, every element of the
    // image's block has been stored once
    nms_pack_finish(pk, bimg, N, cnt, lane, 64);
    return;
  }
  if (lane == 0) out_count[bimg] = cnt;
}

void launch_soft_nms_pack(const float* boxes, const float* scores, int B,
                          int N, float sigma, float score_th, float conf,
                          NmsPack pk) {
  auto s = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(soft_nms_kernel<true>, dim3(B), dim3(64), 0, s, boxes,
      scores, (int*)nullptr, (float*)nullptr, (int*)nullptr, N, sigma,
      score_th, conf, pk);
  HIP_CHECK_LAST();
}

static void launch_soft_nms(const torch::Tensor& b, const torch::Tensor& sc,
                            torch::Tensor& idx, torch::Tensor& osc,
                            torch::Tensor& cnt, int B, int N, double sigma,
                            double score_th, double conf_th) {
  auto s = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(soft_nms_kernel<false>, dim3(B), dim3(64), 0, s,
      b.data_ptr<float>(), sc.data_ptr<float>(), idx.data_ptr<int>(),
      osc.data_ptr<float>(), cnt.data_ptr<int>(), N, (float)sigma,
      (float)score_th, (float)conf_th,
      NmsPack{nullptr, nullptr, nullptr, 0});
  HIP_CHECK_LAST();
}

// batched: one kernel for all images, no host sync (graph-capturable).
// -> idx (B,N) int32 original indices in selection order, out_scores (B,N)
// decayed scores at selection time, counts (B) int32; tails are 0.
std::vector<torch::Tensor> soft_nms_batched(torch::Tensor boxes,
                                            torch::Tensor scores,
                                            double sigma, double score_th,
                                            double conf_th) {
  auto b = boxes.to(at::kFloat).contiguous();
  auto sc = scores.to(at::kFloat).contiguous();
  TORCH_CHECK(b.dim() == 3 && sc.dim() == 2 && b.size(2) == 4 &&
              b.size(0) == sc.size(0) && b.size(1) == sc.size(1),
              "soft_nms_batched: (B,N,4)/(B,N)");
  const int B = b.size(0), N = b.size(1);
  TORCH_CHECK(N <= NMS_CAP, "soft_nms_batched: N > cap");
  auto idx = torch::zeros({B, N}, b.options().dtype(at::kInt));
  auto osc = torch::zeros({B, N}, b.options());
  auto cnt = torch::zeros({B}, b.options().dtype(at::kInt));
  if (N == 0 || B == 0) return {idx, osc, cnt};
  launch_soft_nms(b, sc, idx, osc, cnt, B, N, sigma, score_th, conf_th);
  return {idx, osc, cnt};
}

// single image, the soft twin of nms_fwd: every candidate takes part.
// -> (keep int64 (K), rescored f32 (K)) in selection order.
std::vector<torch::Tensor> soft_nms_fwd(torch::Tensor boxes,
                                        torch::Tensor scores, double sigma,
                                        double score_th) {
  auto b = boxes.to(at::kFloat).contiguous();
  auto sc = scores.to(at::kFloat).contiguous();
  TORCH_CHECK(b.dim() == 2 && b.size(1) == 4 && sc.dim() == 1 &&
              b.size(0) == sc.size(0), "soft_nms: (N,4)/(N)");
  const int N = b.size(0);
  TORCH_CHECK(N <= NMS_CAP,
              "soft_nms: too many boxes (", N, " > ", NMS_CAP, ")");
  if (N == 0)
    return {torch::empty({0}, b.options().dtype(at::kLong)),
            torch::empty({0}, b.options())};
  auto idx = torch::zeros({N}, b.options().dtype(at::kInt));
  auto osc = torch::zeros({N}, b.options());
  auto cnt = torch::zeros({1}, b.options().dtype(at::kInt));
  launch_soft_nms(b, sc, idx, osc, cnt, 1, N, sigma, score_th,
                  -std::numeric_limits<double>::infinity());
  const int k = cnt.item<int>();  // host sync: result used on host
  return {idx.narrow(0, 0, k).to(at::kLong), osc.narrow(0, 0, k)};
}

}  // namespace rthd
