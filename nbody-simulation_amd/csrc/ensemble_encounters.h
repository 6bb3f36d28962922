// Encounters of an ensemble (nbody_encounters_*): per target its nearest source and its clamped pairs, per world one
// nbody_world_encounters, from one call, for all eight ensemble handles, and the pure-host restatement behind
// nbody_encounters_of_f32 / _of_f64.  Internal.  A segment's targets are one world's bodies or one world's tracers; its sources
// are that world's bodies.  Its record and rows are a function of its own rows and of its limit and of nothing else.
//
// Arithmetic.  The handle's precision T, the step's own expressions (pair.h, main.rs:234-253): dx = xj - xi, dy = yj - yi,
// sum = |dx| + |dy|, d2 = dx*dx + dy*dy, each one IEEE operation in T, nothing contracted (the library is built with
// -ffp-contract=off).  A pair is live when `sum` is a normal number, close when it is live and d2 < limit.
//
// Order.  Every output is order-free: the counts are integer sums; a target's nn_d2 is a minimum and its nn_index the lowest
// source index that attains it (a walk over j ascending that replaces on a strict `<` gives exactly that, and so does any
// split of the sources into chunks walked in ascending order); the world's min_* and max_nn_* are extremes with the lowest row
// on a tie.  encounters_of below is that sentence in host code.  The kernels (ensemble_encounters.hip): one 256-thread block per
// (world, tile of 256 targets), one target per lane, the world's source positions staged through LDS in chunks of
// kEncounterChunk; then one block per world that reduces its targets' rows to the record.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <limits>

#include "../../include/nbody_hip.h"
#include "ensemble_rows.h"

namespace nbody {

constexpr int kEncounterBlock = 256;     // targets per tile: one lane each
constexpr int kEncounterChunk = 1024;    // source positions staged in LDS at a time: 8 KB in f32, 16 KB in f64
constexpr int kEncounterFields = 12;     // 8-byte fields of nbody_world_encounters
static_assert(sizeof(nbody_world_encounters) == 8 * kEncounterFields, "12 fields of 8 bytes, no padding");

// The tiles of a segment of n targets (a segment without targets has none: its record comes from the reduce alone).
__host__ __device__ inline uint32_t encounter_tiles(uint32_t n) { return (n + (uint32_t)kEncounterBlock - 1) / (uint32_t)kEncounterBlock; }

struct EncounterArgs {
  const void* pos = nullptr;    // T2 rows of all worlds (the handle's current buffer): the sources, and the targets of the bodies' call
  const void* tpos = nullptr;   // tracers (may be NULL where no world has one)
  const WorldRanges* table = nullptr;     // ragged: one per world (device); NULL: uniform
  const uint32_t* tile_base = nullptr;   // ragged: [n_worlds + 1], the first tile of every world's addressed segment and the total
  const float* limit2 = nullptr;         // [n_worlds] (device) or NULL: limit_all in every world
  float limit_all = 0.0f;
  uint32_t n_bodies = 0, n_tracers = 0;  // uniform: per world
  uint32_t n_worlds = 0;
  uint32_t tiles = 0;           // uniform: the tiles of every world's segment (set by the launch)
  uint32_t tracers = 0;         // the targets are the tracers, not the bodies
  // per target row of all worlds, laid out as the targets are (device); nn_d2 holds T
  int32_t* nn_index = nullptr;
  void* nn_d2 = nullptr;
  uint32_t* close = nullptr;
  uint32_t* live = nullptr;
};

// All worlds' rows and records on `s`: out[n_worlds] (device).  n_tiles: the tiles of all addressed segments together.  Always
// two launches.  Arguments that do not fit come back as hipErrorInvalidValue, never as a launch.
template <class T>
hipError_t launch_ensemble_encounters(hipStream_t s, EncounterArgs a, int64_t n_tiles, nbody_world_encounters* out);

// ---- the host restatement: one segment by the contract above.  self: source j is target j itself and is not a pair.  The
// three per-target arrays may be NULL.
template <class T>
void encounters_of(int64_t n_targets, const T* target, int64_t n_sources, const T* source, bool self, T limit2, nbody_world_encounters* out,
                   int32_t* nn_index, T* nn_d2, uint32_t* close) {
  const double inf = std::numeric_limits<double>::infinity();
  nbody_world_encounters r{};
  r.rows = n_targets;
  r.sources = n_sources;
  r.min_row = r.min_source = r.max_nn_row = -1;
  r.min_d2 = inf;
  r.max_nn_d2 = 0.0;
  for (int64_t i = 0; i < n_targets; ++i) {
    const T xi = target[2 * i], yi = target[2 * i + 1];
    T best = std::numeric_limits<T>::infinity();
    int64_t idx = -1, live = 0, near = 0;
    for (int64_t j = 0; j < n_sources; ++j) {
      if (self && j == i) continue;
      const T dx = source[2 * j] - xi;
      const T dy = source[2 * j + 1] - yi;
      const T sum = std::fabs(dx) + std::fabs(dy);
      if (!std::isnormal(sum)) continue;
      const T d2 = dx * dx + dy * dy;
      ++live;
      if (d2 < limit2) ++near;
      if (idx < 0 || d2 < best) {  // (the first live pair stands even where its d2 overflowed to +inf)
        best = d2;
        idx = j;
      }
    }
    if (nn_index) nn_index[i] = (int32_t)idx;
    if (nn_d2) nn_d2[i] = best;
    if (close) close[i] = (uint32_t)near;
    r.live_pairs += live;
    r.skipped_pairs += n_sources - (self ? 1 : 0) - live;
    r.close_pairs += near;
    if (near) ++r.close_rows;
    if (idx < 0) {
      ++r.isolated_rows;
      continue;
    }
    const double d = (double)best;
    if (r.min_row < 0 || d < r.min_d2) {  // (rows ascend: a tie keeps the lower row)
      r.min_row = i;
      r.min_source = idx;
      r.min_d2 = d;
    }
    if (r.max_nn_row < 0 || d > r.max_nn_d2) {
      r.max_nn_row = i;
      r.max_nn_d2 = d;
    }
  }
  *out = r;
}

}  // namespace nbody
