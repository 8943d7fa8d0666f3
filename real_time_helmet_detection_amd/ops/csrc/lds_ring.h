// Rotation of the 3-deep LDS ring of lds_async.h. Plain C++ with no HIP or
// torch dependency, so the host walks (tests/halo_geo_check.h) replay the
// ring through the functions the kernels call.
#pragma once

#if defined(__HIPCC__)
#define RING_HD __host__ __device__ inline
#else
#define RING_HD inline
#endif

namespace rthd {

// step s reads buffer b, step s + 1 the next one, and the loads of step
// s + 2 go to the one before b
RING_HD int ring3_next(int buf) { return buf == 2 ? 0 : buf + 1; }
RING_HD int ring3_prev(int buf) { return buf == 0 ? 2 : buf - 1; }

}  // namespace rthd
