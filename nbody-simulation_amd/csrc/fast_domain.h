// FAST's domain and clamp floor: the one place that says which coordinates and which clamps the FAST kernels take.  Internal.
//
// A coordinate is inside the domain when it is finite, below kFastBig in magnitude, and zero or at least kFastTiny: inside it
// no pair of the FAST arithmetic overflows or loses a difference to a subnormal.  Everything that routes a body, a target or a
// tracer between FAST and EXACT — on the host or on the device — asks outside_fast(), so the routes agree bit for bit.  (The
// f32 step's own hazard scan and nf_insert, direct_kernels.hip / nearfar.hip, spell the same test inline with these constants.)
#pragma once
#include <hip/hip_runtime.h>

namespace nbody {

constexpr float kFastBig = 1152921504606846976.0f;   // 2^60
constexpr float kFastTiny = 2.384185791015625e-07f;  // 2^-22
constexpr double kFastBig64 = 0x1p100;
constexpr double kFastTiny64 = 0x1p-300;
// f32 FAST's zero-distance bias needs clamp >= 2^-19 (HISTORY.md §4.1); a smaller clamp (or a NaN) always takes EXACT.
constexpr float kFastClampFloor = 1.9073486328125e-06f;

// (a NaN fails the first test)
__host__ __device__ inline bool outside_fast(float v) {
  const float a = __builtin_fabsf(v);
  return !(a < kFastBig) || (a != 0.f && a < kFastTiny);
}
__host__ __device__ inline bool outside_fast(double v) {
  const double a = __builtin_fabs(v);
  return !(a < kFastBig64) || (a != 0.0 && a < kFastTiny64);
}

}  // namespace nbody
