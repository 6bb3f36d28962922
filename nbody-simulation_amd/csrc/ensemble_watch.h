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
//
// A watched sweep (nbody_wsweep_*) gives every world a sampling schedule of its own — a stride, a number of steps after which
// the world stands still and is not looked at again, and sample 0 left out or not — while one launch still samples all worlds.
// Both kernels have a second instantiation for it that reads one WatchWorld per world: a work item whose world does not take
// the launch's sample is skipped by its whole block before anything is staged, `first` is the world's own first taken sample,
// and the reduce takes the world's number of samples from its entry and writes the empty rows of a world that took none.  The
// plain watch keeps the instantiation without a table (WatchEvery: an empty struct, nothing of it is read).  watch_schedule
// below is the host's half: the refusals, the entries, and at which s any world samples at all.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <unordered_map>
#include <vector>

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

// A world's schedule in a watched sweep: it takes sample s iff first <= s <= steps and s % stride == 0.  16 bytes, read once per
// work item by a scalar load.
struct WatchWorld {
  int32_t stride;    // >= 1
  int32_t steps;     // the world's own steps of the call: no sample after them
  uint32_t first;    // its first taken sample (0, or with NBODY_WATCH_RESUME its stride); NBODY_WATCH_NEVER: it takes none
  uint32_t samples;  // how many it takes
};
static_assert(sizeof(WatchWorld) == 16, "one 16-byte load per work item");
struct WatchEvery {};  // the plain watch: every world takes every launch's sample
struct WatchTable {
  const WatchWorld* worlds;  // [n_worlds] (device)
};

// The schedules of a watched sweep on the host.  check() is every refusal that steps[], stride[] and n_steps can earn, with the
// world at fault; build() fills the entries (NULL: the caller wants the union alone) and keeps, per distinct stride, the largest
// steps[k] among its worlds, so that any(s) — does at least one world take sample s — costs one test per distinct stride and
// the whole call O(n_worlds + n_steps * distinct strides), whatever the number of samples.  A stride above n_steps samples at 0
// alone, whatever it is: all of them count as one.
struct WatchSchedule {
  enum Refusal { kOk = 0, kNoWorld, kBadFlags, kBadSteps, kStepOutside, kBadStride };
  static Refusal check(int64_t n_worlds, const int32_t* steps, int n_steps, const int32_t* stride, uint32_t flags, int64_t* world) {
    if (n_worlds < 1) return kNoWorld;
    if (flags & ~(NBODY_WATCH_TRACERS | NBODY_WATCH_RESUME)) return kBadFlags;
    if (n_steps < 0) return kBadSteps;
    for (int64_t k = 0; k < n_worlds; ++k) {
      *world = k;
      if (steps && (steps[k] < 0 || steps[k] > n_steps)) return kStepOutside;
      if (stride && stride[k] < 1) return kBadStride;
    }
    return kOk;
  }
  static WatchWorld world(int32_t steps, int32_t stride, bool resume) {
    WatchWorld w;
    w.stride = stride;
    w.steps = steps;
    const int64_t taken = (int64_t)(steps / stride) + (resume ? 0 : 1);
    w.samples = (uint32_t)taken;
    w.first = taken ? (resume ? (uint32_t)stride : 0u) : NBODY_WATCH_NEVER;
    return w;
  }
  void build(int64_t n_worlds, const int32_t* steps, int n_steps, const int32_t* stride, uint32_t flags, WatchWorld* entries) {
    resume = (flags & NBODY_WATCH_RESUME) != 0;
    std::unordered_map<int32_t, size_t> slot;
    strides.clear();
    for (int64_t k = 0; k < n_worlds; ++k) {
      const int32_t st = steps ? steps[k] : n_steps, sd = stride ? stride[k] : 1;
      if (entries) entries[k] = world(st, sd, resume);
      const int32_t key = sd > n_steps ? INT32_MAX : sd;  // (s % key == 0 at s = 0 alone for every s <= n_steps)
      const auto at = slot.find(key);
      if (at == slot.end()) {
        slot.emplace(key, strides.size());
        strides.push_back({key, st});
      } else if (strides[at->second].second < st) {
        strides[at->second].second = st;
      }
    }
  }
  bool any(int s) const {
    if (s == 0 && resume) return false;
    for (const auto& d : strides)
      if (s <= d.second && s % d.first == 0) return true;
    return false;
  }
  bool resume = false;
  std::vector<std::pair<int32_t, int32_t>> strides;  // (stride, the most steps of a world with it)
};

// One sample of all worlds on `s`.  `a` as the encounters take it (its per-row outputs are not used); n_tiles: the tiles of all
// addressed segments together; nothing is launched for 0.  per_lane: 1 or 2 (the product build has kWatchPerLane alone).
// Arguments that do not fit come back as hipErrorInvalidValue, never as a launch.
// sched (device, [n_worlds]): NULL for the plain watch; with it w.first is not read and a world is sampled by its own entry.
template <class T>
hipError_t launch_ensemble_watch_sample(hipStream_t s, EncounterArgs a, const WatchRun& w, int64_t n_tiles, int per_lane,
                                        const WatchWorld* sched = nullptr);

// The records from the running rows: out[n_worlds] (device).  samples: how many samples the call took; with 0 the rows are not
// read (they were never written).  One launch.  With sched every world's number comes from its entry, `samples` is not read, and
// the rows of a world that took none are written here: +inf, -1, NEVER, NEVER, 0, NEVER.
template <class T>
hipError_t launch_ensemble_watch_worlds(hipStream_t s, EncounterArgs a, const WatchRun& w, uint32_t samples, nbody_world_watch* out,
                                        const WatchWorld* sched = nullptr);

}  // namespace nbody
