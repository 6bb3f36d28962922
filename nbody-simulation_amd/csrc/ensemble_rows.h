// Where a world's rows are, for the calls that read every world of an ensemble (ensemble_frames.h, ensemble_summary.h,
// ensemble_encounters.h).  Internal.  A uniform handle (n_bodies, n_tracers the same in every world) computes a world's row ranges
// from its index; a ragged one reads them from a table, one WorldRanges per world, which the driver builds from the sizes and
// counts it holds (ens_world_table, ensemble_observers.h).  The lookups below are shared where the kernels that use them compile
// to what they compiled to with a helper of their own; frame_world (ensemble_frames.hip: 32-bit products) and encounter_rows
// (ensemble_encounter_device.h: sources and targets from one load of the record) stay apart for that reason.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace nbody {

struct WorldRanges {  // a ragged world's rows (16 bytes: the device reads it as one uint4)
  uint32_t row0, n;   // bodies: rows [row0, row0 + n) of pos / vel / mass
  uint32_t trow0, m;  // tracers: rows [trow0, trow0 + m) of tpos / tvel; m == 0: none
};

// The world of a work item: the last world whose base is not past the item.  base[0 .. n_worlds) ascends; a world without items
// shares its base with the next and is skipped.  The same in every lane of a block.
__device__ __forceinline__ uint32_t world_of_item(const uint32_t* base, uint32_t n_worlds, uint64_t item) {
  uint32_t lo = 0, hi = n_worlds - 1;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (base[mid] <= item) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// A world's bodies (tracers == 0) or tracers: from the table (ragged) or from its index (uniform: table == NULL).
__device__ __forceinline__ void world_segment(const WorldRanges* table, uint32_t n_bodies, uint32_t n_tracers, uint32_t tracers, uint32_t world,
                                              size_t& row0, uint32_t& n) {
  if (table) {
    const uint4 w = reinterpret_cast<const uint4*>(table)[world];
    row0 = tracers ? w.z : w.x;
    n = tracers ? w.w : w.y;
  } else {
    n = tracers ? n_tracers : n_bodies;
    row0 = (size_t)world * n;  // (rows of all worlds <= 2^26)
  }
}

}  // namespace nbody
