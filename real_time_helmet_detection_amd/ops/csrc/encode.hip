// Device-side input pipeline: CenterNet target encoding and uint8 image
// normalisation (the two training-step stages the dataloader workers did in
// numpy: transform.box2hm per sample and utils.Normalizer per image).
//
// encode_targets — a GATHER, not a scatter. Threads own output elements
// (four consecutive x of one row of one plane group) and loop over the
// image's objects, which are staged through LDS in chunks of ENC_CHUNK with
// the per-object parameters (centre cell, integer radius, gaussian
// denominator, offset, size) computed once per object per block. Every
// element of all num_cls+5 planes is written, zeros included, so there is
// no memset and no atomic: the output is bitwise deterministic, the object
// order only matters where box2hm makes it matter (later row wins the
// offset/size of a shared centre cell), and the launch is legal under
// stream capture. N is unbounded (the chunk loop).
//
// Oracle quirks reproduced (transform.box2hm / draw_gaussian):
//   - per-object arithmetic in fp32 in the oracle's order: /scale first,
//     centre = (max+min)/2; no fma contraction (numpy has none)
//   - centre cell = truncation toward zero, so a centre in (-1,0) lands in
//     cell 0 with a negative offset; a centre cell off the map skips the
//     object entirely
//   - radius = centre-to-corner distance, r = (int)radius, window
//     |dx|<=r && |dy|<=r clipped to the map, max-combined per class
//   - the gaussian denominator 2*sigma^2 (sigma = radius/3) is formed in
//     double from the fp32 radius and rounded to fp32 once, as numpy does
//     when it divides the fp32 patch by the python float
// One deliberate difference: a zero-radius box (NaN in the oracle) writes a
// single 1.0 at its centre so no NaN can reach the loss.
//
// normalize_u8 — purely elementwise on the NHWC byte stream: each lane
// reads 3*PX bytes (PX pixels), looks every byte up in a 3x256 table held
// in LDS, and writes three 16-byte vectors. The table is built on the host
// by running the oracle (Normalizer on k/255) once per device, so the fp32
// output is bit-identical to the host path by construction, and the bf16
// table is that table cast by torch, so bf16 == fp32.to(bf16).
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include "common.h"

namespace rthd {

constexpr int ENC_CHUNK = 64;    // objects staged per LDS pass
constexpr int ENC_THREADS = 256;

struct EncObj {  // one staged object (struct-of-arrays in LDS)
  int xi[ENC_CHUNK], yi[ENC_CHUNK], r[ENC_CHUNK], lbl[ENC_CHUNK];
  float den[ENC_CHUNK];
  float xoff[ENC_CHUNK], yoff[ENC_CHUNK], xsz[ENC_CHUNK], ysz[ENC_CHUNK];
};

// Per-object parameters for rows [base, base+ENC_CHUNK) of image b; rows
// past N, padding rows (label < 0) and skipped objects get lbl = -1.
DEV_INLINE void enc_stage(EncObj& o, const float* __restrict__ boxes,
                          const int* __restrict__ labels, int64_t row0,
                          int base, int N, int h, int w, float sf,
                          int num_cls, bool normalized) {
#pragma clang fp contract(off)
  const int t = threadIdx.x;
  if (t >= ENC_CHUNK) return;
  int lbl = -1;
  const int n = base + t;
  if (n < N) {
    lbl = labels[row0 + n];
    if (lbl >= num_cls) lbl = -1;  // would index past the heatmap planes
  }
  if (lbl >= 0) {
    const float4 bx =
        *reinterpret_cast<const float4*>(boxes + (row0 + n) * 4);
    const float xmin = bx.x / sf, ymin = bx.y / sf;
    const float xmax = bx.z / sf, ymax = bx.w / sf;
    const float xcen = (xmax + xmin) / 2.0f, ycen = (ymax + ymin) / 2.0f;
    // (int)c in [0, dim)  <=>  -1 < c < dim ; NaN fails and is skipped
    if (xcen > -1.0f && xcen < (float)w && ycen > -1.0f && ycen < (float)h) {
      const int xi = (int)xcen, yi = (int)ycen;
      float xoff = xcen - (float)xi, yoff = ycen - (float)yi;
      float xsz = xmax - xmin, ysz = ymax - ymin;
      if (normalized) {
        xoff = xoff / sf;
        yoff = yoff / sf;
        xsz = xsz / (float)w;
        ysz = ysz / (float)h;
      }
      const float ddx = xcen - xmin, ddy = ycen - ymin;
      const float radius = sqrtf(ddx * ddx + ddy * ddy);
      const double sigma = (double)radius / 3.0;
      o.xi[t] = xi;
      o.yi[t] = yi;
      // a window wider than the map is the whole map: clamp before the cast
      o.r[t] = radius < 1e9f ? (int)radius : 1000000000;
      // radius 0: the window is the centre cell alone, -(0)/1 -> exp = 1
      o.den[t] = radius == 0.0f ? 1.0f : (float)(2.0 * sigma * sigma);
      o.xoff[t] = xoff;
      o.yoff[t] = yoff;
      o.xsz[t] = xsz;
      o.ysz[t] = ysz;
    } else {
      lbl = -1;
    }
  }
  o.lbl[t] = lbl;
}

// 16-byte store where the address allows it (always when w % 4 == 0),
// scalar stores for a misaligned group and for the row tail
DEV_INLINE void enc_store4(float* __restrict__ p, const float v[4],
                           int nvalid) {
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  if (nvalid == 4 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    // nontemporal keeps this one dwordx4: as a plain store hipcc merged
    // its last lane with the scalar path into dwordx3 + dword
    const f32x4 q = {v[0], v[1], v[2], v[3]};
    __builtin_nontemporal_store(q, reinterpret_cast<f32x4*>(p));
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < nvalid) p[k] = v[k];
  }
}

// grid = (ceil(h*ceil(w/4) / ENC_THREADS), B, num_cls + 1)
//   z <  num_cls : heatmap plane of class z
//   z == num_cls : offset(2) + size(2) + mask(1) planes
__global__ void __launch_bounds__(ENC_THREADS)
encode_targets_kernel(const float* __restrict__ boxes,   // (B,N,4)
                      const int* __restrict__ labels,    // (B,N)
                      float* __restrict__ hm,            // (B,C,h,w)
                      float* __restrict__ off,           // (B,2,h,w)
                      float* __restrict__ sz,            // (B,2,h,w)
                      float* __restrict__ mask,          // (B,1,h,w)
                      int N, int h, int w, int num_cls, float sf,
                      bool normalized) {
  __shared__ EncObj o;
  const int b = blockIdx.y;
  const int z = blockIdx.z;
  const bool heat = z < num_cls;
  const int w4 = (w + 3) >> 2;
  const int g = blockIdx.x * ENC_THREADS + threadIdx.x;
  const bool live = g < h * w4;
  const int y = live ? g / w4 : 0;
  const int x0 = live ? (g - y * w4) * 4 : 0;
  const int64_t row0 = (int64_t)b * N;

  float a0[4] = {0.f, 0.f, 0.f, 0.f};  // heat | offset x
  float a1[4] = {0.f, 0.f, 0.f, 0.f};  // offset y
  float a2[4] = {0.f, 0.f, 0.f, 0.f};  // size x
  float a3[4] = {0.f, 0.f, 0.f, 0.f};  // size y
  float a4[4] = {0.f, 0.f, 0.f, 0.f};  // mask

  for (int base = 0; base < N; base += ENC_CHUNK) {
    __syncthreads();  // previous chunk fully consumed
    enc_stage(o, boxes, labels, row0, base, N, h, w, sf, num_cls,
              normalized);
    __syncthreads();
    if (!live) continue;
    const int cnt = min(ENC_CHUNK, N - base);
    if (heat) {
      for (int j = 0; j < cnt; ++j) {
        if (o.lbl[j] != z) continue;
        const int r = o.r[j];
        const int dy = y - o.yi[j];
        if (dy > r || -dy > r) continue;
        const int dx0 = x0 - o.xi[j];
        if (dx0 > r || -(dx0 + 3) > r) continue;
        const float den = o.den[j];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int dx = dx0 + k;
          if (dx <= r && -dx <= r) {
            const float fx = (float)dx, fy = (float)dy;
            const float d2 = fx * fx + fy * fy;
            a0[k] = fmaxf(a0[k], expf(-d2 / den));
          }
        }
      }
    } else {
      for (int j = 0; j < cnt; ++j) {
        if (o.lbl[j] < 0 || o.yi[j] != y) continue;
        const int k = o.xi[j] - x0;
        if (k < 0 || k > 3) continue;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          if (kk == k) {  // later rows overwrite: the oracle's order
            a0[kk] = o.xoff[j];
            a1[kk] = o.yoff[j];
            a2[kk] = o.xsz[j];
            a3[kk] = o.ysz[j];
            a4[kk] = 1.0f;
          }
        }
      }
    }
  }
  if (!live) return;

  const int nvalid = min(4, w - x0);
  const int64_t hw = (int64_t)h * w;
  const int64_t px = (int64_t)y * w + x0;
  if (heat) {
    enc_store4(hm + ((int64_t)b * num_cls + z) * hw + px, a0, nvalid);
  } else {
    enc_store4(off + ((int64_t)b * 2 + 0) * hw + px, a0, nvalid);
    enc_store4(off + ((int64_t)b * 2 + 1) * hw + px, a1, nvalid);
    enc_store4(sz + ((int64_t)b * 2 + 0) * hw + px, a2, nvalid);
    enc_store4(sz + ((int64_t)b * 2 + 1) * hw + px, a3, nvalid);
    enc_store4(mask + (int64_t)b * hw + px, a4, nvalid);
  }
}

// objects per LDS pass (the tests build a batch that needs several)
int64_t encode_chunk() { return ENC_CHUNK; }

std::vector<torch::Tensor> encode_targets(torch::Tensor boxes,
                                          torch::Tensor labels, int64_t H,
                                          int64_t W, int64_t scale_factor,
                                          int64_t num_cls, bool normalized) {
  TORCH_CHECK(boxes.is_cuda() && labels.is_cuda(),
              "encode_targets: boxes/labels must be device tensors");
  TORCH_CHECK(boxes.scalar_type() == at::kFloat && boxes.dim() == 3 &&
                  boxes.size(2) == 4,
              "encode_targets: boxes must be (B,N,4) float32");
  TORCH_CHECK(labels.scalar_type() == at::kInt && labels.dim() == 2 &&
                  labels.size(0) == boxes.size(0) &&
                  labels.size(1) == boxes.size(1),
              "encode_targets: labels must be (B,N) int32");
  TORCH_CHECK(scale_factor >= 1 && num_cls >= 1 && num_cls <= 65534,
              "encode_targets: bad scale_factor / num_cls");
  auto boxes_ = boxes.contiguous();
  auto labels_ = labels.contiguous();
  const int64_t B = boxes_.size(0), N = boxes_.size(1);
  const int64_t h = H / scale_factor, w = W / scale_factor;
  TORCH_CHECK(h >= 1 && w >= 1 && h * ((w + 3) / 4) < (1LL << 31) &&
                  N < (1LL << 31) && B <= 65535,
              "encode_targets: shape out of range");

  auto opt = boxes_.options();
  auto hm = torch::empty({B, num_cls, h, w}, opt);
  auto off = torch::empty({B, 2, h, w}, opt);
  auto sz = torch::empty({B, 2, h, w}, opt);
  auto mask = torch::empty({B, 1, h, w}, opt);
  if (B == 0) return {hm, off, sz, mask};

  const int64_t groups = h * ((w + 3) / 4);
  dim3 grid((unsigned)cdiv(groups, ENC_THREADS), (unsigned)B,
            (unsigned)(num_cls + 1));
  auto s = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(encode_targets_kernel, grid, dim3(ENC_THREADS), 0, s,
      boxes_.data_ptr<float>(), labels_.data_ptr<int>(),
      hm.data_ptr<float>(), off.data_ptr<float>(), sz.data_ptr<float>(),
      mask.data_ptr<float>(), (int)N, (int)h, (int)w, (int)num_cls,
      (float)scale_factor, normalized);
  HIP_CHECK_LAST();
  return {hm, off, sz, mask};
}

// ------------------------------ normalize_u8 -------------------------------

template <typename T> struct NormIO;
// fp32: 4 pixels per lane = 12 B in (3 x u32), 48 B out (3 x 16 B)
template <> struct NormIO<float> {
  using word = uint32_t;
  static constexpr int PX = 4;
};
// bf16: 8 pixels per lane = 24 B in (3 x u64), 48 B out (3 x 16 B)
template <> struct NormIO<uint16_t> {
  using word = uint64_t;
  static constexpr int PX = 8;
};

template <typename T>
__global__ void __launch_bounds__(256)
normalize_u8_kernel(const uint8_t* __restrict__ in,
                    const T* __restrict__ table,  // [3][256]
                    T* __restrict__ out, int64_t npix) {
  using IO = NormIO<T>;
  using word = typename IO::word;
  constexpr int PX = IO::PX;
  constexpr int NEL = 3 * PX;              // elements per lane
  constexpr int PER16 = 16 / (int)sizeof(T);  // elements per 16-byte store

  __shared__ T tab[3 * 256];
  for (int i = threadIdx.x; i < 3 * 256; i += blockDim.x) tab[i] = table[i];
  __syncthreads();

  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t ngrp = npix / PX;

  // a group starts on a pixel boundary, so byte k of it is channel k % 3
  const word* in_w = reinterpret_cast<const word*>(in);
  for (int64_t gidx = tid; gidx < ngrp; gidx += stride) {
    word wv[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) wv[i] = in_w[gidx * 3 + i];
    alignas(16) T v[NEL];
#pragma unroll
    for (int k = 0; k < NEL; ++k) {
      const int byte = (int)((wv[k / PX] >> (8 * (k % PX))) & 0xff);
      v[k] = tab[(k % 3) * 256 + byte];
    }
    uint4* o16 = reinterpret_cast<uint4*>(out + gidx * NEL);
#pragma unroll
    for (int i = 0; i < NEL / PER16; ++i)
      o16[i] = *reinterpret_cast<const uint4*>(&v[i * PER16]);
  }

  // tail: the last npix % PX pixels, one element per thread
  const int64_t total = npix * 3;
  for (int64_t e = ngrp * NEL + tid; e < total; e += stride)
    out[e] = tab[(int)(e % 3) * 256 + in[e]];
}

torch::Tensor normalize_u8(torch::Tensor img_u8, torch::Tensor table) {
  TORCH_CHECK(img_u8.is_cuda() && img_u8.scalar_type() == at::kByte &&
                  img_u8.dim() == 4 && img_u8.size(3) == 3,
              "normalize_u8: image must be a (B,H,W,3) uint8 device tensor");
  const bool is_bf16 = table.scalar_type() == at::kBFloat16;
  TORCH_CHECK(table.is_cuda() && table.numel() == 3 * 256 &&
                  (is_bf16 || table.scalar_type() == at::kFloat),
              "normalize_u8: table must be (3,256) float32 or bfloat16");
  auto in_ = img_u8.contiguous();
  // the kernel reads 4/8-byte words: a view at an odd storage offset
  // gets a fresh (aligned) allocation
  if (reinterpret_cast<uintptr_t>(in_.data_ptr()) & 7) in_ = in_.clone();
  auto table_ = table.contiguous();
  // NHWC storage viewed as (B,3,H,W): channels_last strides, no copy
  auto out = torch::empty(in_.sizes(), table_.options());
  const int64_t npix = in_.numel() / 3;
  if (npix > 0) {
    auto s = at::cuda::getCurrentCUDAStream();
    if (is_bf16) {
      const int grid = ew_grid(cdiv(npix, NormIO<uint16_t>::PX), 256);
      hipLaunchKernelGGL(normalize_u8_kernel<uint16_t>, dim3(grid),
          dim3(256), 0, s, in_.data_ptr<uint8_t>(),
          reinterpret_cast<const uint16_t*>(table_.data_ptr()),
          reinterpret_cast<uint16_t*>(out.data_ptr()), npix);
    } else {
      const int grid = ew_grid(cdiv(npix, NormIO<float>::PX), 256);
      hipLaunchKernelGGL(normalize_u8_kernel<float>, dim3(grid), dim3(256),
          0, s, in_.data_ptr<uint8_t>(), table_.data_ptr<float>(),
          out.data_ptr<float>(), npix);
    }
    HIP_CHECK_LAST();
  }
  return out.permute({0, 3, 1, 2});
}

}  // namespace rthd
