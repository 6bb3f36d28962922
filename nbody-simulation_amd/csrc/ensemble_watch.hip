// A watched run of an ensemble: the sampling pass and the reduce behind nbody_watch_* (ensemble_watch.h says what a sample is
// and why closeness comes from the minimum; include/nbody_ensemble.h states the contract).
//
// ensemble_watch_sample: the encounters' decomposition (ensemble_encounters.hip) — one block per (world, tile of 256 targets)
// work item, a grid of at most 2^20 blocks striding over the items, the world's source positions through LDS in chunks of
// kEncounterChunk with NaN past the last source, 16-byte broadcast reads, j ascending and a strict `<` — with a leaner pair:
// two subtractions, |.| + |.|, two products and a sum, the class test, one compare and two selects.  There is no `live` and
// no `close` counter, and no test for the body's own row: its differences are +0 or NaN, `sum` is not a normal number, and the
// class test drops it as it drops a coincident body.  kPerLane targets per lane (tile slots l and l + 256 / kPerLane) in a block
// of 256 / kPerLane lanes: with two, every LDS read serves two pairs.  profiles/ensemble_watch.txt has both; kWatchPerLane
// (ensemble_watch.h) is the one the product launches.  At the end of the item a lane folds (best, idx, sample) into its own
// targets' running rows and evaluates within_bounds of their positions: rows that no other lane touches, in stream order.
// ensemble_watch_worlds: one block per world over its targets' running rows; lane to lane by shuffles, wave to wave through LDS.
// No floating-point atomics; nothing is read back between the launches.
// Both kernels are instantiated twice: over WatchEvery for the plain watch, and over WatchTable for a watched sweep, whose
// worlds keep schedules of their own (ensemble_watch.h).  What differs is behind `if constexpr`: the plain instantiation reads
// no table and is the code it was.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "driver.h"
#include "ensemble_encounter_device.h"
#include "ensemble_watch.h"
#include "env.h"

namespace nbody {

namespace {

// One (target, source) pair by the encounters' contract, keeping the minimum alone: j ascends from call to call.
template <class T> __device__ __forceinline__ void watch_pair(T xi, T yi, T sx, T sy, uint32_t j, T& best, int32_t& idx) {
  const T dx = sx - xi;
  const T dy = sy - yi;
  const T sum = encounter_abs(dx) + encounter_abs(dy);
  const T d2 = dx * dx + dy * dy;
  const bool take = __builtin_isnormal(sum) & ((d2 < best) | (idx < 0));  // (the first live pair stands even at d2 = +inf)
  best = take ? d2 : best;
  idx = take ? (int32_t)j : idx;
}

// A target's sample folded into its running row.  (best, idx): the sample's nearest live source, idx < 0: none.
// first: this is the first taken sample of the target's world in the call.
template <class T>
__device__ __forceinline__ void watch_fold(const WatchRun& w, uint32_t first, size_t row, T best, int32_t idx, T limit, bool out) {
  T* const min_d2 = reinterpret_cast<T*>(w.min_d2);
  const bool has = idx >= 0;
  const bool close = has & (best < limit);  // (a NaN or zero limit is never close; a live d2 is never NaN)
  if (first) {
    min_d2[row] = best;  // (+inf, -1 without a live pair)
    w.min_index[row] = idx;
    w.min_sample[row] = has ? w.sample : NBODY_WATCH_NEVER;
    w.first_close[row] = close ? w.sample : NBODY_WATCH_NEVER;
    w.close_samples[row] = close ? 1u : 0u;
    w.first_out[row] = out ? w.sample : NBODY_WATCH_NEVER;
    return;
  }
  if (has && (w.min_index[row] < 0 || best < min_d2[row])) {  // (a later sample replaces on a strict `<` only)
    min_d2[row] = best;
    w.min_index[row] = idx;
    w.min_sample[row] = w.sample;
  }
  if (close) {
    if (w.first_close[row] == NBODY_WATCH_NEVER) w.first_close[row] = w.sample;
    w.close_samples[row] += 1u;
  }
  if (out && w.first_out[row] == NBODY_WATCH_NEVER) w.first_out[row] = w.sample;
}

// Does the world of a work item take the launch's sample w.sample, and is it the world's first?  The world is the same in every
// lane of the block, so its entry arrives by one scalar load and the answer is the block's.
__device__ __forceinline__ bool watch_takes(const WatchTable& t, const WatchRun& w, uint32_t world, bool& first) {
  const uint4 e = reinterpret_cast<const uint4*>(t.worlds)[__builtin_amdgcn_readfirstlane(world)];  // (says "uniform" to the compiler)
  first = w.sample == e.z;
  return w.sample >= e.z && w.sample <= e.y && w.sample % e.x == 0u;  // (first = NEVER: never; steps < 2^31 as unsigned)
}

template <class T, int kPerLane, class Sched>
__global__ __launch_bounds__(kEncounterBlock / kPerLane) void ensemble_watch_sample(const EncounterArgs a, const WatchRun w, uint64_t n_items,
                                                                                    const Sched sched) {
  using T2 = typename EncounterTypes<T>::Vec2;
  constexpr int kThreads = kEncounterBlock / kPerLane;
  __shared__ __attribute__((aligned(16))) T2 staged[kEncounterChunk];
  const uint32_t l = threadIdx.x;
  const T2* const pos = reinterpret_cast<const T2*>(a.pos);
  const T2* const targets = a.tracers ? reinterpret_cast<const T2*>(a.tpos) : pos;
  const T h = (T)w.height;  // (<= 2^24: exact)

  for (uint64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
    const EncounterSeg s = encounter_item(a, item);
    uint32_t first = w.first;
    if constexpr (!std::is_same_v<Sched, WatchEvery>) {
      bool own_first;
      if (!watch_takes(sched, w, s.world, own_first)) continue;  // (the whole block: before any staging or barrier)
      first = own_first ? 1u : 0u;
    }
    const T limit = encounter_limit<T>(a, s.world);
    uint32_t t[kPerLane];
    T xi[kPerLane], yi[kPerLane], best[kPerLane];
    int32_t idx[kPerLane];
#pragma unroll
    for (int r = 0; r < kPerLane; ++r) {
      t[r] = s.tile * (uint32_t)kEncounterBlock + l + (uint32_t)(kThreads * r);
      xi[r] = yi[r] = 0;
      if (t[r] < s.n_tgt) {
        const T2 p = targets[s.tgt0 + t[r]];
        xi[r] = p.x;
        yi[r] = p.y;
      }
      best[r] = (T)__builtin_huge_val();
      idx[r] = -1;
    }
    const bool valid = t[0] < s.n_tgt;  // (the lane's first slot is its lowest target)
    for (uint32_t c0 = 0; c0 < s.n_src; c0 += (uint32_t)kEncounterChunk) {
      __syncthreads();  // (every lane is done with the chunk before, or with the item before)
      encounter_stage<T, kThreads>(staged, pos, s, c0, l);
      __syncthreads();
      const uint32_t count = valid ? encounter_chunk_count(s, c0) : 0u;  // whole groups of four
      for (uint32_t jj = 0; jj < count; jj += 4) {
        const uint32_t j = c0 + jj;
        if constexpr (sizeof(T) == 4) {
          const float4 q0 = reinterpret_cast<const float4*>(staged)[jj / 2], q1 = reinterpret_cast<const float4*>(staged)[jj / 2 + 1];
#pragma unroll
          for (int r = 0; r < kPerLane; ++r) {
            watch_pair<T>(xi[r], yi[r], q0.x, q0.y, j, best[r], idx[r]);
            watch_pair<T>(xi[r], yi[r], q0.z, q0.w, j + 1, best[r], idx[r]);
            watch_pair<T>(xi[r], yi[r], q1.x, q1.y, j + 2, best[r], idx[r]);
            watch_pair<T>(xi[r], yi[r], q1.z, q1.w, j + 3, best[r], idx[r]);
          }
        } else {
          const T2 q0 = staged[jj], q1 = staged[jj + 1], q2 = staged[jj + 2], q3 = staged[jj + 3];
#pragma unroll
          for (int r = 0; r < kPerLane; ++r) {
            watch_pair<T>(xi[r], yi[r], q0.x, q0.y, j, best[r], idx[r]);
            watch_pair<T>(xi[r], yi[r], q1.x, q1.y, j + 1, best[r], idx[r]);
            watch_pair<T>(xi[r], yi[r], q2.x, q2.y, j + 2, best[r], idx[r]);
            watch_pair<T>(xi[r], yi[r], q3.x, q3.y, j + 3, best[r], idx[r]);
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kPerLane; ++r) {
      if (t[r] >= s.n_tgt) continue;
      const bool inside = yi[r] < h && xi[r] < h && yi[r] >= (T)0 && xi[r] >= (T)0;  // within_bounds; NaN fails
      watch_fold<T>(w, first, s.tgt0 + t[r], best[r], idx[r], limit, !inside);
    }
  }
}

// What a lane, a wave or a block knows of a world's targets over the call.
struct WatchPart {
  uint64_t close_rows, close_row_samples, out_rows, isolated;
  uint32_t first_close, first_out, min_sample;  // NBODY_WATCH_NEVER: none (the largest uint32: a minimum ignores it)
  int64_t min_row;                              // -1: no target with a live pair yet
  double min_d2;
};
__device__ __forceinline__ WatchPart watch_nothing() {
  return WatchPart{0, 0, 0, 0, NBODY_WATCH_NEVER, NBODY_WATCH_NEVER, NBODY_WATCH_NEVER, -1, __builtin_huge_val()};
}

// The smaller (d2, sample, row): a total order, so the join is associative and commutative.
__device__ __forceinline__ void watch_join(WatchPart& p, const WatchPart& o) {
  p.close_rows += o.close_rows;
  p.close_row_samples += o.close_row_samples;
  p.out_rows += o.out_rows;
  p.isolated += o.isolated;
  p.first_close = o.first_close < p.first_close ? o.first_close : p.first_close;
  p.first_out = o.first_out < p.first_out ? o.first_out : p.first_out;
  if (o.min_row >= 0 &&
      (p.min_row < 0 || o.min_d2 < p.min_d2 ||
       (o.min_d2 == p.min_d2 && (o.min_sample < p.min_sample || (o.min_sample == p.min_sample && o.min_row < p.min_row))))) {
    p.min_row = o.min_row;
    p.min_sample = o.min_sample;
    p.min_d2 = o.min_d2;
  }
}

__device__ __forceinline__ WatchPart watch_from_lane(const WatchPart& p, int d) {
  WatchPart o;
  o.close_rows = (uint64_t)__shfl_xor((long long)p.close_rows, d, 64);
  o.close_row_samples = (uint64_t)__shfl_xor((long long)p.close_row_samples, d, 64);
  o.out_rows = (uint64_t)__shfl_xor((long long)p.out_rows, d, 64);
  o.isolated = (uint64_t)__shfl_xor((long long)p.isolated, d, 64);
  o.first_close = (uint32_t)__shfl_xor((int)p.first_close, d, 64);
  o.first_out = (uint32_t)__shfl_xor((int)p.first_out, d, 64);
  o.min_sample = (uint32_t)__shfl_xor((int)p.min_sample, d, 64);
  o.min_row = (int64_t)__shfl_xor((long long)p.min_row, d, 64);
  o.min_d2 = __shfl_xor(p.min_d2, d, 64);
  return o;
}

__device__ __forceinline__ int64_t watch_sample_or_none(uint32_t s) { return s == NBODY_WATCH_NEVER ? -1 : (int64_t)s; }

template <class T, class Sched>
__global__ __launch_bounds__(kEncounterBlock) void ensemble_watch_worlds(const EncounterArgs a, const WatchRun w, uint32_t samples_all,
                                                                         nbody_world_watch* __restrict__ out, const Sched sched) {
  __shared__ WatchPart waves[kEncounterBlock / 64];
  const uint32_t l = threadIdx.x;
  T* const min_d2 = reinterpret_cast<T*>(w.min_d2);
  for (uint32_t world = blockIdx.x; world < a.n_worlds; world += gridDim.x) {
    EncounterSeg s;
    encounter_rows(a, world, s);
    uint32_t samples = samples_all;
    if constexpr (!std::is_same_v<Sched, WatchEvery>) samples = sched.worlds[world].samples;
    WatchPart p = watch_nothing();
    for (uint32_t t = l; t < s.n_tgt; t += (uint32_t)kEncounterBlock) {
      const size_t row = s.tgt0 + t;
      if (!samples) {  // (no sample was taken: the rows were never written)
        ++p.isolated;
        if constexpr (!std::is_same_v<Sched, WatchEvery>) {  // a world among others that took some: its rows are the empty ones
          min_d2[row] = (T)__builtin_huge_val();
          w.min_index[row] = -1;
          w.min_sample[row] = NBODY_WATCH_NEVER;
          w.first_close[row] = NBODY_WATCH_NEVER;
          w.close_samples[row] = 0u;
          w.first_out[row] = NBODY_WATCH_NEVER;
        }
        continue;
      }
      const uint32_t near = w.close_samples[row], fc = w.first_close[row], fo = w.first_out[row];
      p.close_rows += near ? 1u : 0u;
      p.close_row_samples += near;
      p.out_rows += fo != NBODY_WATCH_NEVER ? 1u : 0u;
      p.first_close = fc < p.first_close ? fc : p.first_close;
      p.first_out = fo < p.first_out ? fo : p.first_out;
      if (w.min_index[row] < 0) {
        ++p.isolated;
        continue;
      }
      const double d = (double)min_d2[row];  // (exact)
      const uint32_t at = w.min_sample[row];
      if (p.min_row < 0 || d < p.min_d2 || (d == p.min_d2 && at < p.min_sample)) {  // (rows ascend in a lane: the lower row stands)
        p.min_row = t;
        p.min_sample = at;
        p.min_d2 = d;
      }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) watch_join(p, watch_from_lane(p, d));
    __syncthreads();  // (lane 0 is done with `waves` of the world before)
    if ((l & 63u) == 0) waves[l >> 6] = p;
    __syncthreads();
    if (l == 0) {
      WatchPart v = waves[0];
      for (int k = 1; k < kEncounterBlock / 64; ++k) watch_join(v, waves[k]);
      nbody_world_watch r;
      r.rows = s.n_tgt;
      r.sources = s.n_src;
      r.samples = samples;
      r.min_row = v.min_row;
      r.min_source = v.min_row >= 0 ? w.min_index[s.tgt0 + (size_t)v.min_row] : -1;
      r.min_sample = v.min_row >= 0 ? (int64_t)v.min_sample : -1;
      r.min_d2 = v.min_d2;
      r.close_rows = (int64_t)v.close_rows;
      r.close_row_samples = (int64_t)v.close_row_samples;
      r.first_close_sample = watch_sample_or_none(v.first_close);
      r.out_rows = (int64_t)v.out_rows;
      r.first_out_sample = watch_sample_or_none(v.first_out);
      r.isolated_rows = (int64_t)v.isolated;
      out[world] = r;
    }
  }
}

// The launches' own checks of `a`, and its tiles per world where the worlds are of one size.
hipError_t watch_args(EncounterArgs& a, int64_t n_tiles) {
  if (a.n_worlds < 1 || (int64_t)a.n_worlds > (1ll << 26) || !a.pos || n_tiles < 0 || n_tiles > (1ll << 27)) return hipErrorInvalidValue;
  if (a.table) {
    a.tiles = 0;
    if (!a.tile_base) return hipErrorInvalidValue;
  } else {
    a.tile_base = nullptr;
    a.tiles = encounter_tiles(a.tracers ? a.n_tracers : a.n_bodies);
    const uint64_t rows = (uint64_t)(a.tracers ? a.n_tracers : a.n_bodies) * a.n_worlds;
    if (a.n_bodies < 1 || (uint64_t)a.n_bodies * a.n_worlds > (1ull << 26) || rows > (1ull << 26) || n_tiles != (int64_t)a.n_worlds * a.tiles)
      return hipErrorInvalidValue;
  }
  return hipSuccess;
}

bool watch_rows_missing(const WatchRun& w) {
  return !w.min_d2 || !w.min_index || !w.min_sample || !w.first_close || !w.close_samples || !w.first_out;
}

}  // namespace

template <class T>
hipError_t launch_ensemble_watch_sample(hipStream_t s, EncounterArgs a, const WatchRun& w, int64_t n_tiles, int per_lane, const WatchWorld* sched) {
  if (hipError_t h = watch_args(a, n_tiles)) return h;
  if (n_tiles == 0) return hipSuccess;
  if (watch_rows_missing(w) || (a.tracers && !a.tpos) || w.height > kWatchMaxHeight) return hipErrorInvalidValue;
  const unsigned grid = (unsigned)(n_tiles < (int64_t)kEncounterMaxGrid ? n_tiles : (int64_t)kEncounterMaxGrid);
  if (sched) {  // a watched sweep: the product's targets per lane in both builds
    hipLaunchKernelGGL((ensemble_watch_sample<T, kWatchPerLane, WatchTable>), dim3(grid), dim3(kEncounterBlock / kWatchPerLane), 0, s, a, w,
                       (uint64_t)n_tiles, WatchTable{sched});
  } else if (per_lane == kWatchPerLane) {
    hipLaunchKernelGGL((ensemble_watch_sample<T, kWatchPerLane, WatchEvery>), dim3(grid), dim3(kEncounterBlock / kWatchPerLane), 0, s, a, w,
                       (uint64_t)n_tiles, WatchEvery{});
  } else if (kLabBuild && (per_lane == 1 || per_lane == 2)) {
    if constexpr (kLabBuild)
      hipLaunchKernelGGL((ensemble_watch_sample<T, 3 - kWatchPerLane, WatchEvery>), dim3(grid), dim3(kEncounterBlock / (3 - kWatchPerLane)), 0, s, a,
                         w, (uint64_t)n_tiles, WatchEvery{});
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

template <class T>
hipError_t launch_ensemble_watch_worlds(hipStream_t s, EncounterArgs a, const WatchRun& w, uint32_t samples, nbody_world_watch* out,
                                        const WatchWorld* sched) {
  if (!out || a.n_worlds < 1 || (int64_t)a.n_worlds > (1ll << 26)) return hipErrorInvalidValue;
  if (a.table ? !a.tile_base : a.n_bodies < 1) return hipErrorInvalidValue;
  const uint64_t rows = a.table ? 0 : (uint64_t)(a.tracers ? a.n_tracers : a.n_bodies) * a.n_worlds;  // (a table's rows: its builder knows them)
  if ((samples || sched) && rows && watch_rows_missing(w)) return hipErrorInvalidValue;
  const unsigned grid = a.n_worlds < kEncounterMaxGrid ? a.n_worlds : kEncounterMaxGrid;
  if (sched)
    hipLaunchKernelGGL((ensemble_watch_worlds<T, WatchTable>), dim3(grid), dim3(kEncounterBlock), 0, s, a, w, 0u, out, WatchTable{sched});
  else
    hipLaunchKernelGGL((ensemble_watch_worlds<T, WatchEvery>), dim3(grid), dim3(kEncounterBlock), 0, s, a, w, samples, out, WatchEvery{});
  return hipGetLastError();
}

template hipError_t launch_ensemble_watch_sample<float>(hipStream_t, EncounterArgs, const WatchRun&, int64_t, int, const WatchWorld*);
template hipError_t launch_ensemble_watch_sample<double>(hipStream_t, EncounterArgs, const WatchRun&, int64_t, int, const WatchWorld*);
template hipError_t launch_ensemble_watch_worlds<float>(hipStream_t, EncounterArgs, const WatchRun&, uint32_t, nbody_world_watch*, const WatchWorld*);
template hipError_t launch_ensemble_watch_worlds<double>(hipStream_t, EncounterArgs, const WatchRun&, uint32_t, nbody_world_watch*, const WatchWorld*);

}  // namespace nbody
