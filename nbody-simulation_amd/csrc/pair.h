// The reference's pair function (calculate_gravity, src/main.rs:234-253) in f32 and f64, and the FAST
// pairs beside it: shared by the tree walks (tree_kernels.hip) and the f64 direct step (direct64.hip).  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include "div_pair.h"

namespace nbody {

template <class T> struct V2;
template <> struct V2<float> { using type = float2; };
template <> struct V2<double> { using type = double2; };
template <class T> struct V4;
template <> struct V4<float> { using type = float4; };
template <> struct V4<double> { using type = double4; };

template <class T> __device__ __forceinline__ bool is_normal_t(T v) { return __builtin_isnormal(v); }

template <class T>
__device__ __forceinline__ void pair_as_written(T px, T py, T qx, T qy, T force, T clamp, T& ax, T& ay) {
  T dx = qx - px;                                        // main.rs:236
  T dy = qy - py;
  T sum = __builtin_fabs(dx) + __builtin_fabs(dy);       // :238
  if (!is_normal_t(sum)) return;                         // :241-243
  T distance = dx * dx + dy * dy;                        // :245
  // :247-249 as one max (half the cost of compare + select): `distance` is never NaN here (a normal `sum` means finite
  // dx, dy), and for a NaN clamp both forms keep `distance`
  distance = __builtin_fmax(distance, clamp);
  T den = sum * distance;
  ax = ax + (dx * force) / den;                          // :252
  ay = ay + (dy * force) / den;
}
template <>
__device__ __forceinline__ void pair_as_written<float>(float px, float py, float qx, float qy, float force,
                                                       float clamp, float& ax, float& ay) {
  float dx = qx - px;
  float dy = qy - py;
  float sum = __builtin_fabsf(dx) + __builtin_fabsf(dy);
  if (!__builtin_isnormal(sum)) return;
  float distance = dx * dx + dy * dy;
  distance = __builtin_fmaxf(distance, clamp);
  float den = sum * distance;
  const float2 q = div_pair(dx * force, dy * force, den);  // the two quotients of :252, their multiply-adds packed (div_pair.h)
  ax = ax + q.x;
  ay = ay + q.y;
}

// FAST pair for the walk (opt-in, nbody_arith FAST): one reciprocal instead of two IEEE divisions, fused
// multiply-adds; a zero difference contributes exactly 0 through the biased denominator (direct_kernels.hip).  The
// node tests are untouched, so a target interacts with exactly the reference's list of nodes and particles; only
// the rounding of each term differs (tolerance of tests/_tol.py, not bit parity).
__device__ __forceinline__ void pair_fast(float px, float py, float qx, float qy, float force, float clamp, float& ax,
                                          float& ay) {
  float dx = qx - px, dy = qy - py;
  float sum = __builtin_fabsf(dx) + __builtin_fabsf(dy);
  float d2 = __builtin_fmaxf(__builtin_fmaf(dy, dy, dx * dx), clamp);
  float s = force * __builtin_amdgcn_rcpf(__builtin_fmaf(sum, d2, 8.0779356694631609e-28f));  // 2^-90
  ax = __builtin_fmaf(dx, s, ax);
  ay = __builtin_fmaf(dy, s, ay);
}
__device__ __forceinline__ void pair_fast(double px, double py, double qx, double qy, double force, double clamp,
                                          double& ax, double& ay) {
  double dx = qx - px, dy = qy - py;
  double sum = __builtin_fabs(dx) + __builtin_fabs(dy);
  double d2 = __builtin_fmax(__builtin_fma(dy, dy, dx * dx), clamp);
  double den = __builtin_fma(sum, d2, 0x1p-700);
  double r = __builtin_amdgcn_rcp(den);          // ~27 bits
  r = __builtin_fma(__builtin_fma(-den, r, 1.0), r, r);   // Newton: ~54 bits
  double s = force * r;
  ax = __builtin_fma(dx, s, ax);
  ay = __builtin_fma(dy, s, ay);
}

// calculate_gravity (main.rs:234-253) up to, but not including, the `+=`: a pair the reference skips is -0.0, the
// identity of IEEE addition.
template <class T> __device__ __forceinline__ typename V2<T>::type pair_term_t(T px, T py, T qx, T qy, T force, T clamp) {
  using T2 = typename V2<T>::type;
  const T dx = qx - px;
  const T dy = qy - py;
  const T sum = __builtin_fabs(dx) + __builtin_fabs(dy);
  if (!is_normal_t(sum)) return T2{(T)-0.0, (T)-0.0};
  T distance = dx * dx + dy * dy;
  distance = sizeof(T) == 8 ? (T)__builtin_fmax((double)distance, (double)clamp) : (T)__builtin_fmaxf((float)distance, (float)clamp);
  const T den = sum * distance;
  if constexpr (sizeof(T) == 4) {
    const float2 q = div_pair((float)(dx * force), (float)(dy * force), (float)den);
    return T2{(T)q.x, (T)q.y};
  }
  return T2{(dx * force) / den, (dy * force) / den};
}

// pair_term_t<double> without the branch: both divisions are evaluated for every pair and a skipped pair's quotients are
// replaced by -0.0 — the same bits, in straight-line code, so the division chains of a block of pairs interleave (with the
// branch every pair runs under its own exec mask, one chain after the other).
__device__ __forceinline__ double2 pair_term_select(double px, double py, double qx, double qy, double force, double clamp) {
  const double dx = qx - px;
  const double dy = qy - py;
  const double sum = __builtin_fabs(dx) + __builtin_fabs(dy);
  const bool keep = is_normal_t(sum);
  const double distance = __builtin_fmax(dx * dx + dy * dy, clamp);
  const double den = sum * distance;
  const double tx = (dx * force) / den, ty = (dy * force) / den;
  return double2{keep ? tx : -0.0, keep ? ty : -0.0};
}

}  // namespace nbody
