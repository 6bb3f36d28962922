// Encounters of an ensemble: per target its nearest source and its clamped pairs, per world one nbody_world_encounters
// (ensemble_encounters.h states the arithmetic and why every output is order-free), and nbody_encounters_of_f32 / _of_f64, the
// same contract in host code.
//
// ensemble_encounter_pairs: one 256-thread block per (world, tile of 256 targets) work item; a grid of at most 2^20 blocks
// strides over the items.  Lane l holds target 256 tile + l in registers.  The world's source positions go through LDS in chunks
// of 1024 (8 KB in f32, 16 KB in f64: far below what the step kernels stage, so LDS does not set the occupancy); slots past the
// last source hold NaN, which no pair survives, so the walk runs over whole groups of four.  Every lane reads the same address —
// a broadcast, 16 bytes per read: two sources in f32, one in f64 — and walks j ascending, replacing on a strict `<`: the lowest
// j of a tie stands.  Per pair: two subtractions, |.| + |.|, two products and a sum, a class test, two compares; no division, no
// transcendental, no fma.  One target per lane, not two: per source a wave spends some twelve vector instructions and half a
// 16-byte LDS read, so with four SIMDs on one LDS the reads take a small share of the cycles already, and a second target would
// buy nothing but registers.  A wave whose lanes are all past the last target skips the walk and keeps the barriers.
// ensemble_encounter_worlds: one block per world over its targets' rows: integer sums and the two extremes, joined lane to lane
// by shuffles and wave to wave through LDS.  The join is associative and commutative (a total order on (d2, row)), so its
// shape is free.  No floating-point atomics; nothing is read back between the launches.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "driver.h"
#include "ensemble_encounter_device.h"
#include "ensemble_encounters.h"

namespace nbody {

namespace {

// One (target, source) pair by the contract: j ascends from call to call.
template <class T>
__device__ __forceinline__ void encounter_pair(T xi, T yi, T sx, T sy, uint32_t j, uint32_t self, T limit, T& best, int32_t& idx, uint32_t& live,
                                               uint32_t& near) {
  const T dx = sx - xi;
  const T dy = sy - yi;
  const T sum = encounter_abs(dx) + encounter_abs(dy);
  const T d2 = dx * dx + dy * dy;
  const bool ok = __builtin_isnormal(sum) & (j != self);
  live += ok ? 1u : 0u;
  near += (ok & (d2 < limit)) ? 1u : 0u;
  const bool take = ok & ((d2 < best) | (idx < 0));  // (the first live pair stands even where its d2 overflowed to +inf)
  best = take ? d2 : best;
  idx = take ? (int32_t)j : idx;
}

template <class T>
__global__ __launch_bounds__(kEncounterBlock) void ensemble_encounter_pairs(const EncounterArgs a, uint64_t n_items) {
  using T2 = typename EncounterTypes<T>::Vec2;
  __shared__ __attribute__((aligned(16))) T2 staged[kEncounterChunk];
  const uint32_t l = threadIdx.x;
  const T2* const pos = reinterpret_cast<const T2*>(a.pos);
  const T2* const targets = a.tracers ? reinterpret_cast<const T2*>(a.tpos) : pos;

  for (uint64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
    const EncounterSeg s = encounter_item(a, item);
    const uint32_t t = s.tile * (uint32_t)kEncounterBlock + l;
    const bool valid = t < s.n_tgt;
    const uint32_t self = a.tracers ? 0xffffffffu : t;  // (a source index is below 4096)
    const T limit = encounter_limit<T>(a, s.world);
    T xi = 0, yi = 0;
    if (valid) {
      const T2 p = targets[s.tgt0 + t];
      xi = p.x;
      yi = p.y;
    }
    T best = (T)__builtin_huge_val();
    int32_t idx = -1;
    uint32_t live = 0, near = 0;
    for (uint32_t c0 = 0; c0 < s.n_src; c0 += (uint32_t)kEncounterChunk) {
      __syncthreads();  // (every lane is done with the chunk before, or with the item before)
      encounter_stage<T, kEncounterBlock>(staged, pos, s, c0, l);
      __syncthreads();
      const uint32_t count = valid ? encounter_chunk_count(s, c0) : 0u;  // whole groups of four
      for (uint32_t jj = 0; jj < count; jj += 4) {
        const uint32_t j = c0 + jj;
        if constexpr (sizeof(T) == 4) {
          const float4 q0 = reinterpret_cast<const float4*>(staged)[jj / 2], q1 = reinterpret_cast<const float4*>(staged)[jj / 2 + 1];
          encounter_pair<T>(xi, yi, q0.x, q0.y, j, self, limit, best, idx, live, near);
          encounter_pair<T>(xi, yi, q0.z, q0.w, j + 1, self, limit, best, idx, live, near);
          encounter_pair<T>(xi, yi, q1.x, q1.y, j + 2, self, limit, best, idx, live, near);
          encounter_pair<T>(xi, yi, q1.z, q1.w, j + 3, self, limit, best, idx, live, near);
        } else {
          const T2 q0 = staged[jj], q1 = staged[jj + 1], q2 = staged[jj + 2], q3 = staged[jj + 3];
          encounter_pair<T>(xi, yi, q0.x, q0.y, j, self, limit, best, idx, live, near);
          encounter_pair<T>(xi, yi, q1.x, q1.y, j + 1, self, limit, best, idx, live, near);
          encounter_pair<T>(xi, yi, q2.x, q2.y, j + 2, self, limit, best, idx, live, near);
          encounter_pair<T>(xi, yi, q3.x, q3.y, j + 3, self, limit, best, idx, live, near);
        }
      }
    }
    if (valid) {
      const size_t row = s.tgt0 + t;
      a.nn_index[row] = idx;
      reinterpret_cast<T*>(a.nn_d2)[row] = best;
      a.close[row] = near;
      a.live[row] = live;
    }
  }
}

// What a lane, a wave or a block knows of a world's targets.
struct EncounterPart {
  uint64_t live, close, close_rows, isolated;
  int64_t min_row, max_row;  // -1: no target with a neighbour yet
  double min_d2, max_d2;
};
__device__ __forceinline__ EncounterPart encounter_nothing() { return EncounterPart{0, 0, 0, 0, -1, -1, __builtin_huge_val(), 0.0}; }

// The smaller (d2, row) and the larger d2 with the lower row: a total order, so the join is associative and commutative.
__device__ __forceinline__ void encounter_join(EncounterPart& p, const EncounterPart& o) {
  p.live += o.live;
  p.close += o.close;
  p.close_rows += o.close_rows;
  p.isolated += o.isolated;
  if (o.min_row >= 0 && (p.min_row < 0 || o.min_d2 < p.min_d2 || (o.min_d2 == p.min_d2 && o.min_row < p.min_row))) {
    p.min_row = o.min_row;
    p.min_d2 = o.min_d2;
  }
  if (o.max_row >= 0 && (p.max_row < 0 || o.max_d2 > p.max_d2 || (o.max_d2 == p.max_d2 && o.max_row < p.max_row))) {
    p.max_row = o.max_row;
    p.max_d2 = o.max_d2;
  }
}

__device__ __forceinline__ EncounterPart encounter_from_lane(const EncounterPart& p, int d) {
  EncounterPart o;
  o.live = (uint64_t)__shfl_xor((long long)p.live, d, 64);
  o.close = (uint64_t)__shfl_xor((long long)p.close, d, 64);
  o.close_rows = (uint64_t)__shfl_xor((long long)p.close_rows, d, 64);
  o.isolated = (uint64_t)__shfl_xor((long long)p.isolated, d, 64);
  o.min_row = (int64_t)__shfl_xor((long long)p.min_row, d, 64);
  o.max_row = (int64_t)__shfl_xor((long long)p.max_row, d, 64);
  o.min_d2 = __shfl_xor(p.min_d2, d, 64);
  o.max_d2 = __shfl_xor(p.max_d2, d, 64);
  return o;
}

template <class T>
__global__ __launch_bounds__(kEncounterBlock) void ensemble_encounter_worlds(const EncounterArgs a, nbody_world_encounters* __restrict__ out) {
  __shared__ EncounterPart waves[kEncounterBlock / 64];
  const uint32_t l = threadIdx.x;
  const T* const nn_d2 = reinterpret_cast<const T*>(a.nn_d2);
  for (uint32_t world = blockIdx.x; world < a.n_worlds; world += gridDim.x) {
    EncounterSeg s;
    encounter_rows(a, world, s);
    EncounterPart p = encounter_nothing();
    for (uint32_t t = l; t < s.n_tgt; t += (uint32_t)kEncounterBlock) {  // (rows ascend in a lane: `<` and `>` keep the lower row)
      const size_t row = s.tgt0 + t;
      const uint32_t near = a.close[row];
      p.live += a.live[row];
      p.close += near;
      p.close_rows += near ? 1u : 0u;
      if (a.nn_index[row] < 0) {
        ++p.isolated;
        continue;
      }
      const double d = (double)nn_d2[row];  // (exact)
      if (p.min_row < 0 || d < p.min_d2) {
        p.min_row = t;
        p.min_d2 = d;
      }
      if (p.max_row < 0 || d > p.max_d2) {
        p.max_row = t;
        p.max_d2 = d;
      }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) encounter_join(p, encounter_from_lane(p, d));
    __syncthreads();  // (lane 0 is done with `waves` of the world before)
    if ((l & 63u) == 0) waves[l >> 6] = p;
    __syncthreads();
    if (l == 0) {
      EncounterPart w = waves[0];
      for (int k = 1; k < kEncounterBlock / 64; ++k) encounter_join(w, waves[k]);
      nbody_world_encounters r;
      r.rows = s.n_tgt;
      r.sources = s.n_src;
      r.live_pairs = (int64_t)w.live;
      r.skipped_pairs = (int64_t)s.n_tgt * ((int64_t)s.n_src - (a.tracers ? 0 : 1)) - (int64_t)w.live;
      r.close_pairs = (int64_t)w.close;
      r.close_rows = (int64_t)w.close_rows;
      r.isolated_rows = (int64_t)w.isolated;
      r.min_row = w.min_row;
      r.min_source = w.min_row >= 0 ? a.nn_index[s.tgt0 + (size_t)w.min_row] : -1;
      r.min_d2 = w.min_d2;
      r.max_nn_row = w.max_row;
      r.max_nn_d2 = w.max_d2;
      out[world] = r;
    }
  }
}

}  // namespace

template <class T>
hipError_t launch_ensemble_encounters(hipStream_t s, EncounterArgs a, int64_t n_tiles, nbody_world_encounters* out) {
  if (a.n_worlds < 1 || (int64_t)a.n_worlds > (1ll << 26) || !out || !a.pos || n_tiles < 0 || n_tiles > (1ll << 27)) return hipErrorInvalidValue;
  const uint64_t rows = a.table ? 0 : (uint64_t)(a.tracers ? a.n_tracers : a.n_bodies) * a.n_worlds;
  if (a.table) {
    a.tiles = 0;
    if (!a.tile_base) return hipErrorInvalidValue;
  } else {
    a.tile_base = nullptr;
    a.tiles = encounter_tiles(a.tracers ? a.n_tracers : a.n_bodies);
    if (a.n_bodies < 1 || (uint64_t)a.n_bodies * a.n_worlds > (1ull << 26) || rows > (1ull << 26) || n_tiles != (int64_t)a.n_worlds * a.tiles)
      return hipErrorInvalidValue;
  }
  if (n_tiles > 0 && (!a.nn_index || !a.nn_d2 || !a.close || !a.live || (a.tracers && !a.tpos))) return hipErrorInvalidValue;
  const unsigned pair_grid = (unsigned)(n_tiles < (int64_t)kEncounterMaxGrid ? (n_tiles > 0 ? n_tiles : 1) : (int64_t)kEncounterMaxGrid);
  hipLaunchKernelGGL(ensemble_encounter_pairs<T>, dim3(pair_grid), dim3(kEncounterBlock), 0, s, a, (uint64_t)n_tiles);
  const unsigned world_grid = a.n_worlds < kEncounterMaxGrid ? a.n_worlds : kEncounterMaxGrid;
  hipLaunchKernelGGL(ensemble_encounter_worlds<T>, dim3(world_grid), dim3(kEncounterBlock), 0, s, a, out);
  return hipGetLastError();
}

template hipError_t launch_ensemble_encounters<float>(hipStream_t, EncounterArgs, int64_t, nbody_world_encounters*);
template hipError_t launch_ensemble_encounters<double>(hipStream_t, EncounterArgs, int64_t, nbody_world_encounters*);

}  // namespace nbody

using namespace nbody;

// The contract in host code: no device, no handle.
template <class T>
static int encounters_of_checked(int64_t n_targets, const T* target_xy, int64_t n_sources, const T* source_xy, int self, T limit2,
                                 nbody_world_encounters* out, int32_t* nn_index, T* nn_d2, uint32_t* close) {
  if (n_targets < 0 || n_sources < 0 || !out) return NBODY_ERR_INVALID;
  if ((n_targets > 0 && !target_xy) || (n_sources > 0 && !source_xy)) return NBODY_ERR_INVALID;
  if (self != 0 && n_targets != n_sources) return NBODY_ERR_INVALID;
  if (n_sources > (int64_t)INT32_MAX) return NBODY_ERR_INVALID;  // (nn_index is an int32)
  encounters_of<T>(n_targets, target_xy, n_sources, source_xy, self != 0, limit2, out, nn_index, nn_d2, close);
  return NBODY_OK;
}

NB_API int nbody_encounters_of_f32(int64_t n_targets, const float* target_xy, int64_t n_sources, const float* source_xy, int self, float limit2,
                                   nbody_world_encounters* out, int32_t* nn_index, float* nn_d2, uint32_t* close) {
  return encounters_of_checked<float>(n_targets, target_xy, n_sources, source_xy, self, limit2, out, nn_index, nn_d2, close);
}
NB_API int nbody_encounters_of_f64(int64_t n_targets, const double* target_xy, int64_t n_sources, const double* source_xy, int self, double limit2,
                                   nbody_world_encounters* out, int32_t* nn_index, double* nn_d2, uint32_t* close) {
  return encounters_of_checked<double>(n_targets, target_xy, n_sources, source_xy, self, limit2, out, nn_index, nn_d2, close);
}
