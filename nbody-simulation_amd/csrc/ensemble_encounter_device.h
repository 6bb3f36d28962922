// Device helpers shared by the kernels that walk (world, tile of 256 targets) work items against the world's bodies:
// ensemble_encounters.hip and ensemble_watch.hip.  Internal.  The work item -> (world, tile) mapping, a world's source and target
// rows from one load of its record, the limit of a world, and the staging of one chunk of sources in LDS.  Everything is
// __forceinline__: a kernel that includes this compiles to what it compiled to with these functions in its own unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ensemble_encounters.h"

namespace nbody {

template <class T> struct EncounterTypes;
template <> struct EncounterTypes<float> { using Vec2 = float2; };
template <> struct EncounterTypes<double> { using Vec2 = double2; };

constexpr uint32_t kEncounterMaxGrid = 1u << 20;

struct EncounterSeg {
  uint32_t world, tile;  // the work item
  size_t src0, tgt0;     // the first source row in pos, the first target row in the targets' array and in the per-row outputs
  uint32_t n_src, n_tgt;
};

// A world's sources and addressed targets: from the table (ragged) or from its index (uniform).  Both from one load of the
// record: world_segment (ensemble_rows.h) once per kind would load it twice.
__device__ __forceinline__ void encounter_rows(const EncounterArgs& a, uint32_t world, EncounterSeg& s) {
  if (a.table) {
    const uint4 w = reinterpret_cast<const uint4*>(a.table)[world];
    s.src0 = w.x;
    s.n_src = w.y;
    s.tgt0 = a.tracers ? w.z : w.x;
    s.n_tgt = a.tracers ? w.w : w.y;
  } else {
    s.n_src = a.n_bodies;
    s.src0 = (size_t)world * a.n_bodies;  // (rows of all worlds <= 2^26)
    s.n_tgt = a.tracers ? a.n_tracers : a.n_bodies;
    s.tgt0 = (size_t)world * s.n_tgt;
  }
}

// Work item -> (world, tile).  The same in every lane of a block.
__device__ __forceinline__ EncounterSeg encounter_item(const EncounterArgs& a, uint64_t item) {
  EncounterSeg s;
  if (!a.table) {
    s.world = (uint32_t)(item / a.tiles);
    s.tile = (uint32_t)(item - (uint64_t)s.world * a.tiles);
  } else {  // (a world without tiles shares its base with the next: skipped)
    s.world = world_of_item(a.tile_base, a.n_worlds, item);
    s.tile = (uint32_t)(item - a.tile_base[s.world]);
  }
  encounter_rows(a, s.world, s);
  return s;
}

template <class T> __device__ __forceinline__ T encounter_limit(const EncounterArgs& a, uint32_t world) {
  return (T)(a.limit2 ? a.limit2[world] : a.limit_all);  // (widened on the f64 handles, as a step widens its clamp)
}

__device__ __forceinline__ float encounter_abs(float v) { return __builtin_fabsf(v); }
__device__ __forceinline__ double encounter_abs(double v) { return __builtin_fabs(v); }

// The sources [c0, c0 + kEncounterChunk) of a world into `staged` by a block of kThreads lanes, lane l; slots past the last
// source hold NaN, which no pair survives.  The caller puts a barrier before (the chunk before is done with) and after.
template <class T, int kThreads>
__device__ __forceinline__ void encounter_stage(typename EncounterTypes<T>::Vec2* staged, const typename EncounterTypes<T>::Vec2* pos,
                                                const EncounterSeg& s, uint32_t c0, uint32_t l) {
  using T2 = typename EncounterTypes<T>::Vec2;
  const T nan = (T)__builtin_nanf("");
#pragma unroll
  for (int k = 0; k < kEncounterChunk / kThreads; ++k) {
    const uint32_t slot = l + (uint32_t)kThreads * k, j = c0 + slot;
    staged[slot] = j < s.n_src ? pos[s.src0 + j] : T2{nan, nan};
  }
}

// How many staged slots a lane with a target walks in the chunk at c0: whole groups of four (the NaN fill covers the rest).
__device__ __forceinline__ uint32_t encounter_chunk_count(const EncounterSeg& s, uint32_t c0) {
  const uint32_t left = s.n_src - c0;
  return left < (uint32_t)kEncounterChunk ? (left + 3u) & ~3u : (uint32_t)kEncounterChunk;
}

}  // namespace nbody
