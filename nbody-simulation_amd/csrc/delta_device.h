// Device helpers of the NBD1 encoders (format: delta_codec.h): what the single-sequence encoder of a context
// (delta_snapshot.hip) and the batched encoder of the ensembles (ensemble_deltas.hip) both compute per 64-row block, kept
// in one place so that the two cannot drift apart.  Internal; device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "delta_codec.h"

namespace nbody {

__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v |= (uint32_t)__shfl_xor((int)v, d, 64);
  return v;
}
__device__ __forceinline__ uint64_t wave_or(uint64_t v) {
  return ((uint64_t)wave_or((uint32_t)(v >> 32)) << 32) | wave_or((uint32_t)v);
}
__device__ __forceinline__ int bits_of(uint32_t v) { return 32 - __clz((int)v); }
__device__ __forceinline__ int bits_of(uint64_t v) { return 64 - __clzll((long long)v); }

template <class K> __device__ __forceinline__ void residuals(K cur, K prev, K prev2, K& z0, K& z1) {
  z0 = delta_zigzag((K)(cur - prev));
  z1 = delta_zigzag((K)(cur - (K)(prev + (K)(prev - prev2))));
}

}  // namespace nbody
