// A watched run of an ensemble (nbody_watch_*): per target its closest approach, its close samples and the sample at which it
// left the frame, per world one nbody_world_watch, over the steps of one call, for all eight ensemble handles.  Internal.
// include/nbody_ensemble.h ("a watched run") states the contract; this is how it is laid out on the device.
//
// A sample is one launch of ensemble_watch_sample over the encounters' work items, (world, tile of 256 targets): it evaluates
// the encounters' (nn_d2, nn_index) of every target — the same expressions, the same order, the same tie rule — and folds them
// into the target's running row, six values in six arrays laid out as the targets are.  Closeness is read off the minimum: a
// target has a pair with d2 < limit iff its smallest live d2 is below the limit, so the pair body keeps (best, idx) alone.  A
// row belongs to the one lane that holds its target, and the launches of a call are in stream order: the fold is a plain
// read-modify-write, write-only in the first taken sample.  ensemble_watch_worlds then reduces every world's rows to its record:
// integer sums, minima of sample numbers, and the smallest (d2, sample, row) — a total order, so the shape of the join is free.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/nbody_hip.h"
#include "ensemble_encounters.h"

namespace nbody {

constexpr int kWatchFields = 13;           // 8-byte fields of nbody_world_watch
static_assert(sizeof(nbody_world_watch) == 8 * kWatchFields, "13 fields of 8 bytes, no padding");
constexpr uint32_t kWatchMaxHeight = 1u << 24;  // as the frames' and the summaries'
// Targets per lane of ensemble_watch_sample: two measured faster in f64 (3 % without the rows, 10 % with them) and the same as
// one within the trials' spread in f32 (profiles/ensemble_watch.txt).  The laboratory build instantiates both and reads
// NBODY_WATCH_PER_LANE (1 or 2).
constexpr int kWatchPerLane = 2;

// The running rows of a call (device), one entry per target of all worlds, and what one sample brings to them.
struct WatchRun {
  void* min_d2 = nullptr;          // T
  int32_t* min_index = nullptr;
  uint32_t* min_sample = nullptr;
  uint32_t* first_close = nullptr;
  uint32_t* close_samples = nullptr;
  uint32_t* first_out = nullptr;
  uint32_t sample = 0;             // the sample's number: steps of the call taken so far
  uint32_t first = 0;              // the first taken sample of the call: the rows are written, not read
  uint32_t height = 0;             // the frame of `out`
};

// One sample of all worlds on `s`.  `a` as the encounters take it (its per-row outputs are not used); n_tiles: the tiles of all
// addressed segments together; nothing is launched for 0.  per_lane: 1 or 2 (the product build has kWatchPerLane alone).
// Arguments that do not fit come back as hipErrorInvalidValue, never as a launch.
template <class T> hipError_t launch_ensemble_watch_sample(hipStream_t s, EncounterArgs a, const WatchRun& w, int64_t n_tiles, int per_lane);

// The records from the running rows: out[n_worlds] (device).  samples: how many samples the call took; with 0 the rows are not
// read (they were never written).  One launch.
template <class T> hipError_t launch_ensemble_watch_worlds(hipStream_t s, EncounterArgs a, const WatchRun& w, uint32_t samples, nbody_world_watch* out);

}  // namespace nbody
