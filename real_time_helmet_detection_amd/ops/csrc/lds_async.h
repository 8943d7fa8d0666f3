// Shared primitives of the kernels that fill LDS with global_load_lds into a
// 3-deep ring and read their MFMA fragments with counted waits of their own
// (conv_halo.hip, conv_halo_fp8.hip, wgrad_tr.hip, wgrad_row.hip): the
// inline-asm LDS reads, the counted waits, the ring rotation, and the
// opt-in to more than 64 KB of dynamic LDS.
//
// Why the fragment reads are inline asm. Through the builtin the compiler
// orders every LDS read behind ALL pending global_load_lds with s_waitcnt
// vmcnt(0) (it cannot see that ring buffers are disjoint), which forbids
// loads in flight across a K-step. These kernels place the vmcnt / lgkmcnt
// waits for their reads themselves: wait_vm<N>() plus a raw s_barrier at the
// top of a K-step, wait_lgkm(n) before the MFMAs that consume a fragment,
// and frag_ready() to tie the fragment registers to a point after that wait
// (the asm reads are invisible to the compiler's own wait insertion).
//
// The compiler takes the "=v" result of a read as written when the asm ends,
// while the data lands only at the kernel's lgkmcnt wait. So between a read
// and its wait the compiler must emit nothing that touches the result: no
// v_mov, no v_accvgpr copy, no scratch spill.
// AUDIT ON EVERY EDIT of this header, of a kernel that uses it, or of the
// toolchain: in the .s of that kernel, the lines from the first ds_read of a
// K-step to the s_waitcnt lgkmcnt that covers it hold only the reads, address
// arithmetic on OTHER registers, global_load_lds and MFMAs on already-waited
// fragments; ScratchSize is 0. The last audit of the four kernels is recorded
// in profiles/lds_async_refactor.md; each kernel's GPU test runs many K-steps
// bitwise against an older kernel and fails on such a regression.
#pragma once

#include <mutex>

#include "conv_common.h"
#include "lds_ring.h"

namespace rthd {

using i32x4 = __attribute__((ext_vector_type(4))) int;
using i16x4 = __attribute__((ext_vector_type(4))) short;
typedef __attribute__((address_space(3))) char lds_char;

// ------------------------------ device side ---------------------------------

// 32-bit LDS address of the block's dynamic shared memory
DEV_INLINE uint32_t lds_base(char* smem) {
  return (uint32_t)(uintptr_t)(lds_char*)smem;
}

// ds_read_b128 of 16 B at addr + OFF; T is bf16x8 or i32x4
template <int OFF, typename T>
DEV_INLINE T lds_read_b128(uint32_t addr) {
  static_assert(sizeof(T) == 16, "one 16-B fragment register group");
  T v;
  asm volatile("ds_read_b128 %0, %1 offset:%2"
               : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}

// ds_read_b64_tr_b16 at addr + OFF: one half (4 k-slots) of a 16x16x32 bf16
// operand, transposed on the read
template <int OFF>
DEV_INLINE i16x4 lds_read_tr16_b64(uint32_t addr) {
  i16x4 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2"
               : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}

// wait until at most n LDS reads are outstanding; n is a constant after
// unrolling, 0..15 (the counter's range)
DEV_INLINE void wait_lgkm(int n) {
#define RTHD_LGKM_CASE(N) \
  case N: asm volatile("s_waitcnt lgkmcnt(" #N ")" ::: "memory"); break;
  switch (n) {
    RTHD_LGKM_CASE(0) RTHD_LGKM_CASE(1) RTHD_LGKM_CASE(2) RTHD_LGKM_CASE(3)
    RTHD_LGKM_CASE(4) RTHD_LGKM_CASE(5) RTHD_LGKM_CASE(6) RTHD_LGKM_CASE(7)
    RTHD_LGKM_CASE(8) RTHD_LGKM_CASE(9) RTHD_LGKM_CASE(10) RTHD_LGKM_CASE(11)
    RTHD_LGKM_CASE(12) RTHD_LGKM_CASE(13) RTHD_LGKM_CASE(14) RTHD_LGKM_CASE(15)
    default: __builtin_unreachable();
  }
#undef RTHD_LGKM_CASE
}

// wait until at most N global_load_lds (or other vector memory ops) of this
// wave are outstanding
template <int N>
DEV_INLINE void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// the ring rotation, ring3_next(buf) / ring3_prev(buf), is lds_ring.h's

// the fragment registers v... are complete here (call after the wait_lgkm
// that covers their reads)
template <typename T>
DEV_INLINE void frag_ready(T& v) {
  asm volatile("" : "+v"(v));
}
template <typename T, typename... R>
DEV_INLINE void frag_ready(T& v, R&... rest) {
  frag_ready(v);
  frag_ready(rest...);
}

// ------------------------------- host side ----------------------------------

// A kernel gets 64 KB of dynamic LDS without opting in. Above that, raise
// the kernel's limit once per device. The kernel is a template argument, so
// the once-per-device state is per kernel instantiation (keyed on a type it
// would be shared by instantiations of equal signature).
template <auto KERNEL>
void lds_opt_in(int bytes, const char* who) {
  if (bytes <= 65536) return;
  static std::mutex mu;
  static uint64_t done = 0;   // one bit per device
  int dev = 0;
  TORCH_CHECK(hipGetDevice(&dev) == hipSuccess && dev < 64, who,
              ": bad device");
  std::lock_guard<std::mutex> lk(mu);
  if (!((done >> dev) & 1)) {
    const hipError_t e = hipFuncSetAttribute(
        reinterpret_cast<const void*>(KERNEL),
        hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    TORCH_CHECK(e == hipSuccess, who, ": cannot opt in to ", bytes,
                " B of LDS: ", hipGetErrorString(e));
    done |= (uint64_t)1 << dev;
  }
}

}  // namespace rthd
