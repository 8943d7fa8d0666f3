// Greedy IoU NMS, single-workgroup, bitmask formulation.
//
// Replaces torchvision.ops.nms (reference evaluate.py:174) and the
// scripted export NMS. v1 ran the classic barrier-serialized greedy loop
// (N iterations x __syncthreads + a fixed 2048-wide bitonic sort):
// 110 us for the typical 100-box call. v2:
//   1. bitonic sort desc by (score, -idx) over the next-pow2 >= N width
//      (index-stable, matching the v1 / torch order),
//   2. the full pairwise IoU BITMASK built in parallel (one u64 word =
//      64 candidate pairs per thread-iteration; j > i bits only),
//   3. a wave-resident scan: lane w owns suppression word w; per row i
//      the wave checks liveness and ORs row i's mask words in lockstep —
//      no block barriers in the O(N) part.
// Everything lives in dynamic LDS (sized for the actual N; > 64 KB
// requests opt in via hipFuncSetAttribute). Returns kept indices
// (original numbering) in descending-score order.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <mutex>

#include "nms_common.h"

namespace rthd {

// grid.x = image index (batched form; the single-image entry uses B=1).
// conf: candidates with score < conf are neither suppressors nor output
// (equivalent to filtering before NMS — they sort to the tail).
// PACK: the packed emit of nms_pack (nms_common.h) replaces the index list;
// out_idx / out_count are then unused (null) and LDS holds W more words.
template <bool PACK>
__global__ void nms_kernel(const float* __restrict__ boxes,  // (B,N,4)
                           const float* __restrict__ scores, // (B,N)
                           int* __restrict__ out_idx,        // (B,N)
                           int* __restrict__ out_count,      // (B,)
                           unsigned long long* __restrict__ mask_gb,
                           int N, int P, int W, float thr, float conf,
                           NmsPack pk) {
  const int bimg = blockIdx.x;
  boxes += (int64_t)bimg * N * 4;
  scores += (int64_t)bimg * N;
  if (!PACK) {
    out_idx += (int64_t)bimg * N;
    out_count += bimg;
  }
  unsigned long long* mask_g =
      mask_gb ? mask_gb + (int64_t)bimg * N * W : nullptr;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sx1 = reinterpret_cast<float*>(smem);
  float* sy1 = sx1 + P;
  float* sx2 = sy1 + P;
  float* sy2 = sx2 + P;
  float* ss = sy2 + P;
  int* sidx = reinterpret_cast<int*>(ss + P);
  // the [N][W] pair mask lives in LDS when it fits (N <= 1024), else in
  // a global scratch buffer passed by the host
  unsigned long long* mask = mask_g
      ? mask_g : reinterpret_cast<unsigned long long*>(sidx + P);
  volatile unsigned long long* rem = mask_g
      ? reinterpret_cast<unsigned long long*>(sidx + P)
      : reinterpret_cast<unsigned long long*>(sidx + P) + (int64_t)N * W;

  for (int i = threadIdx.x; i < P; i += blockDim.x) {
    if (i < N) {
      sx1[i] = boxes[i * 4 + 0];
      sy1[i] = boxes[i * 4 + 1];
      sx2[i] = boxes[i * 4 + 2];
      sy2[i] = boxes[i * 4 + 3];
      ss[i] = scores[i];
      sidx[i] = i;
    } else {
      ss[i] = -3.4e38f;
      sidx[i] = 0x7fffffff;
    }
  }
  for (int w = threadIdx.x; w < W; w += blockDim.x) rem[w] = 0ull;
  __syncthreads();

  // ---- bitonic sort desc by (score, -idx) ----
  for (int k2 = 2; k2 <= P; k2 <<= 1) {
    for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
      for (int i = threadIdx.x; i < P / 2; i += blockDim.x) {
        const int a = (i / j2) * (j2 * 2) + (i % j2);
        const int b = a ^ j2;
        if (b > a) {
          const bool dirDesc = ((a & k2) == 0);
          const bool a_lt_b = (ss[a] < ss[b]) ||
              (ss[a] == ss[b] && sidx[a] > sidx[b]);
          if (dirDesc == a_lt_b) {
            float t;
            int ti;
            t = ss[a]; ss[a] = ss[b]; ss[b] = t;
            ti = sidx[a]; sidx[a] = sidx[b]; sidx[b] = ti;
            if (sidx[a] < N || sidx[b] < N) {
              t = sx1[a]; sx1[a] = sx1[b]; sx1[b] = t;
              t = sy1[a]; sy1[a] = sy1[b]; sy1[b] = t;
              t = sx2[a]; sx2[a] = sx2[b]; sx2[b] = t;
              t = sy2[a]; sy2[a] = sy2[b]; sy2[b] = t;
            }
          }
        }
      }
      __syncthreads();
    }
  }

  // ---- pairwise IoU bitmask (bits for j > i only) ----
  const int nwords = N * W;
  for (int t = threadIdx.x; t < nwords; t += blockDim.x) {
    const int i = t / W;
    const int w = t % W;
    const float ax1 = sx1[i], ay1 = sy1[i], ax2 = sx2[i], ay2 = sy2[i];
    const float area_a = box_area(ax1, ay1, ax2, ay2);
    unsigned long long m = 0ull;
    const int j0 = w * 64;
    const int jend = min(j0 + 64, N);
    for (int j = max(j0, i + 1); j < jend; ++j) {
      const float iou = box_iou(ax1, ay1, ax2, ay2, area_a, sx1[j], sy1[j],
                                sx2[j], sy2[j]);
      if (iou > thr) m |= 1ull << (j - j0);
    }
    mask[(int64_t)i * W + w] = m;
  }
  __syncthreads();

  // ---- wave-resident greedy scan (wave 0; lane w owns rem[w]) ----
  if (threadIdx.x < 64) {
    const int w = threadIdx.x;
    for (int i = 0; i < N; ++i) {
      if (ss[i] < conf) break;  // sorted desc: tail is all below conf
      const bool alive = ((rem[i >> 6] >> (i & 63)) & 1ull) == 0ull;
      if (alive && w < W) rem[w] |= mask[(int64_t)i * W + w];
    }
  }
  __syncthreads();

  if (!PACK) {
    if (threadIdx.x == 0) {
      int k = 0;
      for (int i = 0; i < N && ss[i] >= conf; ++i)
        if (((rem[i >> 6] >> (i & 63)) & 1ull) == 0ull)
          out_idx[k++] = sidx[i];
      *out_count = k;
    }
    return;
  }

  // ---- packed emit: parallel compaction of the survivors ----
  // The serial loop above emits sorted position i iff every position <= i
  // has score >= conf and i's bit of rem is clear. Per 64-candidate word:
  // ballot the conf test, cut it at its first failure, clear the suppressed
  // bits; a survivor's output slot is the popcount of the words before it
  // plus that of the lower bits of its own word. A wave owns whole words
  // (blockDim is a multiple of 64) and meets in the ballot only; the rest
  // is ordered by the block barrier, not by wave lockstep.
  unsigned long long* kw = const_cast<unsigned long long*>(rem) + W;
  int* kfull = reinterpret_cast<int*>(kw + W);
  for (int w = threadIdx.x >> 6; w < W; w += blockDim.x >> 6) {
    const int i = w * 64 + (threadIdx.x & 63);
    const unsigned long long ok = __ballot(i < N && ss[i] >= conf);
    // bits below the first failing one (all 64 when none fails)
    const unsigned long long lead =
        ~ok == 0ull ? ~0ull : ((1ull << __builtin_ctzll(~ok)) - 1ull);
    if ((threadIdx.x & 63) == 0) {
      kw[w] = lead & ~rem[w];
      kfull[w] = ~ok == 0ull;
    }
  }
  __syncthreads();
  // a word with a failing candidate ends the list: the words after it emit
  // nothing. (The last word of an all-pass image is cut at N by the ballot.)
  int total = 0;   // survivors of the whole image
  int wend = W;    // first word past the list
  for (int w = 0; w < W; ++w) {
    total += __popcll(kw[w]);
    if (!kfull[w]) { wend = w + 1; break; }
  }
  for (int i = threadIdx.x; i < N; i += blockDim.x) {
    const int w = i >> 6, l = i & 63;
    if (w >= wend) break;
    const unsigned long long m = kw[w];
    if (((m >> l) & 1ull) == 0ull) continue;
    int k = __popcll(m & ((1ull << l) - 1ull));
    for (int v = 0; v < w; ++v) k += __popcll(kw[v]);
    nms_pack_record(pk, bimg, N, k, sidx[i], sx1[i], sy1[i], sx2[i], sy2[i],
                    ss[i]);
  }
  nms_pack_finish(pk, bimg, N, total, threadIdx.x, blockDim.x);
}

// shared launch logic for the single-image and batched entries
template <bool PACK>
static void launch_nms(const float* pb, const float* psc, int* pidx,
                       int* pcnt, int B, int N, float thr, float conf,
                       const torch::TensorOptions& opt,
                       NmsPack pk = NmsPack{nullptr, nullptr, nullptr, 0}) {
  int P = 64;
  while (P < N) P <<= 1;
  const int W = (int)cdiv(N, 64);
  const bool lds_mask = N <= 1024;  // [N][W] mask fits beside the arrays
  size_t lds = (size_t)P * 24 + (size_t)W * 8;
  if (lds_mask) lds += (size_t)N * W * 8;
  if (PACK) lds += (size_t)W * 12;  // kw (u64) + kfull (int) per word
  torch::Tensor mask_ws;
  unsigned long long* mg = nullptr;
  if (!lds_mask) {
    mask_ws = torch::empty({(int64_t)B * N * W}, opt.dtype(at::kLong));
    mg = reinterpret_cast<unsigned long long*>(mask_ws.data_ptr());
  }
  if (lds > 65536) {
    static std::once_flag once;
    std::call_once(once, [] {
      (void)hipFuncSetAttribute(
          reinterpret_cast<const void*>(&nms_kernel<PACK>),
          hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    });
  }
  auto s = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(nms_kernel<PACK>, dim3(B), dim3(256), lds, s,
      pb, psc, pidx, pcnt, mg, N, P, W, thr, conf, pk);
  HIP_CHECK_LAST();
}

// soft_nms.hip: the PACK instantiation of soft_nms_kernel
void launch_soft_nms_pack(const float* boxes, const float* scores, int B,
                          int N, float sigma, float score_th, float conf,
                          NmsPack pk);

// Either NMS mode with a packed, fixed-shape result (layout: nms_common.h).
// mode 0 selects what nms_batched selects (original scores), mode 1 what
// soft_nms_batched selects (rescored scores). One launch that writes every
// output element: no memset, no atomics, no host read, no allocation sized
// by data — deterministic and legal under stream capture. count is exact as
// a float because N <= NMS_CAP.
torch::Tensor nms_pack(torch::Tensor boxes, torch::Tensor classes,
                       torch::Tensor scores,
                       c10::optional<torch::Tensor> box_scale, int64_t mode,
                       double iou, double sigma, double score_th,
                       double conf) {
  TORCH_CHECK(boxes.is_cuda() && classes.is_cuda() && scores.is_cuda(),
              "nms_pack: device tensors");
  TORCH_CHECK(mode == 0 || mode == 1, "nms_pack: mode 0 (greedy) or 1 (soft)");
  auto b = boxes.to(at::kFloat).contiguous();
  auto sc = scores.to(at::kFloat).contiguous();
  auto cl = classes.to(at::kLong).contiguous();
  TORCH_CHECK(b.dim() == 3 && b.size(2) == 4 && sc.dim() == 2 &&
              cl.dim() == 2 && b.size(0) == sc.size(0) &&
              b.size(1) == sc.size(1) && cl.size(0) == sc.size(0) &&
              cl.size(1) == sc.size(1),
              "nms_pack: (B,N,4)/(B,N)/(B,N)");
  const int B = b.size(0), N = b.size(1);
  TORCH_CHECK(N <= NMS_CAP, "nms_pack: N > cap (", N, " > ", NMS_CAP, ")");
  NmsPack pk{cl.data_ptr<int64_t>(), nullptr, nullptr, 0};
  torch::Tensor bs;
  if (box_scale.has_value() && box_scale->defined()) {
    bs = box_scale->to(at::kFloat).contiguous();
    TORCH_CHECK(bs.is_cuda() &&
                ((bs.dim() == 1 && bs.size(0) == 4) ||
                 (bs.dim() == 2 && bs.size(0) == B && bs.size(1) == 4)),
                "nms_pack: box_scale must be (4,) or (B,4) on the device");
    pk.scale = bs.data_ptr<float>();
    pk.scale_stride = bs.dim() == 2 ? 4 : 0;
  }
  if (N == 0 || B == 0) return torch::zeros({B, 1, NMS_REC}, b.options());
  auto out = torch::empty({B, 1 + N, NMS_REC}, b.options());
  pk.out = out.data_ptr<float>();
  if (mode == 0)
    launch_nms<true>(b.data_ptr<float>(), sc.data_ptr<float>(), nullptr,
                     nullptr, B, N, (float)iou, (float)conf, b.options(), pk);
  else
    launch_soft_nms_pack(b.data_ptr<float>(), sc.data_ptr<float>(), B, N,
                         (float)sigma, (float)score_th, (float)conf, pk);
  return out;
}

// batched: one kernel, one later host sync for ALL images (the per-image
// loop in Prediction paid a sync per image). conf folds the confidence
// filter into the kernel (uniform N per image).
std::vector<torch::Tensor> nms_batched(torch::Tensor boxes,
                                       torch::Tensor scores,
                                       double iou_threshold,
                                       double conf_th) {
  auto b = boxes.to(at::kFloat).contiguous();
  auto sc = scores.to(at::kFloat).contiguous();
  TORCH_CHECK(b.dim() == 3 && sc.dim() == 2 && b.size(0) == sc.size(0) &&
              b.size(1) == sc.size(1), "nms_batched: (B,N,4)/(B,N)");
  const int B = b.size(0), N = b.size(1);
  TORCH_CHECK(N <= NMS_CAP, "nms_batched: N > cap");
  auto out_idx = torch::zeros({B, std::max(N, 1)},
                              b.options().dtype(at::kInt));
  auto out_count = torch::zeros({B}, b.options().dtype(at::kInt));
  if (N == 0) return {out_idx, out_count};
  launch_nms<false>(b.data_ptr<float>(), sc.data_ptr<float>(),
                    out_idx.data_ptr<int>(), out_count.data_ptr<int>(), B,
                    N, (float)iou_threshold, (float)conf_th, b.options());
  return {out_idx, out_count};
}

torch::Tensor nms_fwd(torch::Tensor boxes, torch::Tensor scores,
                      double iou_threshold) {
  auto b = boxes.to(at::kFloat).contiguous();
  auto sc = scores.to(at::kFloat).contiguous();
  const int N = b.size(0);
  TORCH_CHECK(N <= NMS_CAP,
              "nms: too many boxes (", N, " > ", NMS_CAP,
              ") — raise conf_th or topk split");
  auto out_idx = torch::empty({std::max(N, 1)},
                              b.options().dtype(at::kInt));
  auto out_count = torch::zeros({1}, b.options().dtype(at::kInt));
  if (N == 0) return torch::empty({0}, b.options().dtype(at::kLong));
  launch_nms<false>(b.data_ptr<float>(), sc.data_ptr<float>(),
                    out_idx.data_ptr<int>(), out_count.data_ptr<int>(), 1,
                    N, (float)iou_threshold, -3.4e38f, b.options());
  const int k = out_count.item<int>();  // host sync: result used on host
  return out_idx.narrow(0, 0, k).to(at::kLong);
}

}  // namespace rthd
