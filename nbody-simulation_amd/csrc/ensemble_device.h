// What the two ensemble kernels (ensemble_kernels.hip, ensemble64_kernels.hip) share on the device: the butterfly in which the
// lanes of a target meet, and the integration.  Internal.  Overloads on float and double; a 64-bit value crosses lanes as two
// 32-bit DPP / permlane moves, in the same controls and the same order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace nbody {

__device__ __forceinline__ double ens_join(uint32_t lo, uint32_t hi) {
  return __builtin_bit_cast(double, (uint64_t)lo | ((uint64_t)hi << 32));
}
template <int CTRL> __device__ __forceinline__ float ens_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
template <int CTRL> __device__ __forceinline__ double ens_dpp(double v) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, CTRL, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), CTRL, 0xf, 0xf, true);
  return ens_join((uint32_t)lo, (uint32_t)hi);
}
// v_permlane16_swap / v_permlane32_swap through inline asm, as walk_device.h does (the s_nop covers "VALU writes a VGPR, a
// permlane swap reads it"): with both operands a copy of r, the sum of the two results is r of this row + r of its neighbour
// row (rows 0|1, 2|3), resp. r of this half + r of the other half of the wave.
__device__ __forceinline__ float ens_add_neighbour_row(float r) {
  float a = r, b = r;
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  return a + b;
}
__device__ __forceinline__ float ens_add_other_half(float r) {
  float a = r, b = r;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
  return a + b;
}
// In double, once per 32-bit half: the two results are r of the even and r of the odd row of the pair (resp. of the lower and
// the upper half of the wave), in that order in both — their sum has the same bits in both.
__device__ __forceinline__ double ens_add_neighbour_row(double r) {
  const uint64_t u = __builtin_bit_cast(uint64_t, r);
  uint32_t alo = (uint32_t)u, blo = (uint32_t)u, ahi = (uint32_t)(u >> 32), bhi = (uint32_t)(u >> 32);
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\tv_permlane16_swap_b32 %2, %3" : "+v"(alo), "+v"(blo), "+v"(ahi), "+v"(bhi));
  return ens_join(alo, ahi) + ens_join(blo, bhi);
}
__device__ __forceinline__ double ens_add_other_half(double r) {
  const uint64_t u = __builtin_bit_cast(uint64_t, r);
  uint32_t alo = (uint32_t)u, blo = (uint32_t)u, ahi = (uint32_t)(u >> 32), bhi = (uint32_t)(u >> 32);
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\tv_permlane32_swap_b32 %2, %3" : "+v"(alo), "+v"(blo), "+v"(ahi), "+v"(bhi));
  return ens_join(alo, ahi) + ens_join(blo, bhi);
}
// The total of r over the SPLIT consecutive lanes of a group, in every one of them.
template <int SPLIT, class T> __device__ __forceinline__ T ens_group_sum(T r) {
  if constexpr (SPLIT >= 2) r = r + ens_dpp<0xB1>(r);    // quad_perm [1,0,3,2]
  if constexpr (SPLIT >= 4) r = r + ens_dpp<0x4E>(r);    // quad_perm [2,3,0,1]
  if constexpr (SPLIT >= 8) r = r + ens_dpp<0x141>(r);   // row_half_mirror
  if constexpr (SPLIT >= 16) r = r + ens_dpp<0x128>(r);  // row_ror:8
  if constexpr (SPLIT >= 32) r = ens_add_neighbour_row(r);
  if constexpr (SPLIT >= 64) r = ens_add_other_half(r);
  return r;
}

// main.rs:419-423 in the precision of Args (EnsembleArgs, Ensemble64Args), multiply then add, no contraction (TU flag); `row`
// is the body's row among all worlds.
template <class Args, class T> __device__ __forceinline__ void ens_integrate(const Args& a, size_t row, T px, T py, T ax, T ay) {
  using Vec2 = std::remove_pointer_t<decltype(a.vel)>;
  if (a.acc_out) a.acc_out[row] = Vec2{ax, ay};
  if (a.vel) {
    Vec2 v = a.vel[row];
    v.x = v.x + ax * a.delta;
    v.y = v.y + ay * a.delta;
    const T sx = v.x * a.delta, sy = v.y * a.delta;
    a.vel[row] = v;
    a.pos_out[row] = Vec2{px + sx, py + sy};
  }
}

}  // namespace nbody
