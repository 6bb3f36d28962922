// Summaries of an ensemble: one nbody_world_summary per world (ensemble_summary.h states the arithmetic and the order of every
// sum), and nbody_summary_of_f32 / _of_f64, the same contract in host code.
//
// ensemble_summary_chunks: one 256-thread block per (world, chunk of 4096 rows) work item; a grid of at most 2^20 blocks strides
// over the items.  Lane l is chain l of the chunk: it reads rows l + 256 i, i = 0 .. 15 (coalesced float2 / double2 loads) and
// keeps sixteen 8-byte accumulators in registers: the six ordered chains, the mass, six order-free keys (summary_key: integers
// that order as the doubles do) and three counts.  Then the tree of the contract: P[l] + P[l + 128] and P[l] + P[l + 64] through
// LDS (the upper half writes, the lower half reads and adds), strides 32 .. 1 as xor shuffles in wave 0 — lane l < s receives
// P[l + s], and IEEE addition commutes, so every node is the contract's node.  Lane 0 writes the record.
// ensemble_summary_combine: where a segment has several chunks (tracers only), one lane per (world, field) walks that world's
// chunk records in ascending order.  No floating-point atomics; nothing is read back between the launches.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "driver.h"
#include "ensemble_summary.h"

namespace nbody {

namespace {

template <class T> struct SummaryTypes;
template <> struct SummaryTypes<float> { using Vec2 = float2; using Mass = float; };
template <> struct SummaryTypes<double> { using Vec2 = double2; using Mass = uint32_t; };

// The accumulators of a lane, in the order their kinds need: [0, kMass] are doubles that add, then keys that take a minimum,
// keys that take a maximum, and counts.
enum : int { kWx, kWy, kWvx, kWvy, kWv2, kSep2, kMass, kMinX, kMinY, kMaxX, kMaxY, kSpeed, kSepMax, kCounted, kInBounds, kSepRows, kAcc };
constexpr uint32_t kSummaryMaxGrid = 1u << 20;

__device__ __forceinline__ uint64_t sum_bits(double v) { return __builtin_bit_cast(uint64_t, v); }
__device__ __forceinline__ double sum_real(uint64_t b) { return __builtin_bit_cast(double, b); }

// Accumulator f of two lanes joined.  f is a constant wherever this is called (unrolled loops).
__device__ __forceinline__ uint64_t summary_join(int f, uint64_t a, uint64_t b) {
  if (f <= kMass) return sum_bits(sum_real(a) + sum_real(b));
  if (f <= kMinY) return (uint64_t)((int64_t)a < (int64_t)b ? (int64_t)a : (int64_t)b);
  if (f <= kSepMax) return (uint64_t)((int64_t)a > (int64_t)b ? (int64_t)a : (int64_t)b);
  return a + b;
}

struct SummarySeg {
  uint32_t world, chunk;  // the work item
  size_t row0;            // the segment's first row in its arrays
  uint32_t n;             // its rows
};

// A world's addressed segment: from the table (ragged) or from its index (uniform).
__device__ __forceinline__ void summary_rows(const SummaryArgs& a, uint32_t world, size_t& row0, uint32_t& n) {
  world_segment(a.table, a.n_bodies, a.n_tracers, a.tracers, world, row0, n);
}

// The first chunk record of a world among those of all worlds.
__device__ __forceinline__ uint64_t summary_first_chunk(const SummaryArgs& a, uint32_t world) {
  if (!a.table) return (uint64_t)world * a.chunks;
  return a.chunk_base ? a.chunk_base[world] : world;  // (ragged bodies: one chunk per world)
}

// Work item -> (world, chunk).  The same in every lane of a block.
__device__ __forceinline__ SummarySeg summary_item(const SummaryArgs& a, uint64_t item) {
  SummarySeg s;
  if (!a.table) {
    s.world = (uint32_t)(item / a.chunks);
    s.chunk = (uint32_t)(item - (uint64_t)s.world * a.chunks);
  } else if (!a.chunk_base) {
    s.world = (uint32_t)item;
    s.chunk = 0;
  } else {  // (every world has at least one chunk: the bases ascend strictly)
    s.world = world_of_item(a.chunk_base, a.n_worlds, item);
    s.chunk = (uint32_t)(item - a.chunk_base[s.world]);
  }
  summary_rows(a, s.world, s.row0, s.n);
  return s;
}

template <class T>
__global__ __launch_bounds__(kSummaryBlock) void ensemble_summary_chunks(const SummaryArgs a, uint64_t n_items, nbody_world_summary* __restrict__ dst) {
  using T2 = typename SummaryTypes<T>::Vec2;
  using Mass = typename SummaryTypes<T>::Mass;
  __shared__ uint64_t upper[kAcc][kSummaryBlock / 2];  // what lanes 128 .. 255 hand to lanes 0 .. 127
  __shared__ uint64_t second[kAcc][64];                // what lanes 64 .. 127 hand to lanes 0 .. 63
  const uint32_t l = threadIdx.x;
  const T2* const pos = reinterpret_cast<const T2*>(a.tracers ? a.tpos : a.pos);
  const T2* const vel = reinterpret_cast<const T2*>(a.tracers ? a.tvel : a.vel);
  const double h = (double)a.height;
  const double inf = __builtin_huge_val();

  for (uint64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
    const SummarySeg s = summary_item(a, item);
    const int32_t j = a.ref ? a.ref[s.world] : -1;
    size_t ref0 = 0;
    if (j >= 0) {
      uint32_t ref_n;
      summary_rows(a, (uint32_t)j, ref0, ref_n);  // (the driver has checked that ref_n == s.n)
    }
    double wx = 0.0, wy = 0.0, wvx = 0.0, wvy = 0.0, wv2 = 0.0, sep2 = 0.0, mass = 0.0;
    int64_t min_x = summary_key(inf), min_y = min_x, max_x = summary_key(-inf), max_y = max_x, speed = summary_key(0.0), sep_max = speed;
    uint64_t counted = 0, in_bounds = 0, sep_rows = 0;
    for (int i = 0; i < kSummaryPerLane; ++i) {
      const uint32_t r = s.chunk * (uint32_t)kSummaryChunk + l + (uint32_t)kSummaryBlock * i;  // (a segment has at most 2^26 rows)
      if (r >= s.n) break;
      const T2 p = pos[s.row0 + r], v = vel[s.row0 + r];
      const double x = (double)p.x, y = (double)p.y, vx = (double)v.x, vy = (double)v.y;
      if (y < h && x < h && y >= 0.0 && x >= 0.0) ++in_bounds;  // within_bounds; NaN fails
      if (!(summary_finite(x) && summary_finite(y) && summary_finite(vx) && summary_finite(vy))) continue;
      const double w = a.tracers ? 1.0 : (double)reinterpret_cast<const Mass*>(a.mass)[s.row0 + r];
      const double v2 = vx * vx + vy * vy;
      ++counted;
      mass += w;
      const int64_t kx = summary_key(x), ky = summary_key(y), kv = summary_key(v2);
      min_x = kx < min_x ? kx : min_x; max_x = kx > max_x ? kx : max_x;
      min_y = ky < min_y ? ky : min_y; max_y = ky > max_y ? ky : max_y;
      speed = kv > speed ? kv : speed;
      wx = wx + w * x;
      wy = wy + w * y;
      wvx = wvx + w * vx;
      wvy = wvy + w * vy;
      wv2 = wv2 + w * v2;
      if (j < 0) continue;
      const T2 rp = pos[ref0 + r], rv = vel[ref0 + r];
      const double rx = (double)rp.x, ry = (double)rp.y;
      if (!(summary_finite(rx) && summary_finite(ry) && summary_finite((double)rv.x) && summary_finite((double)rv.y))) continue;
      const double dx = x - rx, dy = y - ry, d2 = dx * dx + dy * dy;
      const int64_t kd = summary_key(d2);
      ++sep_rows;
      sep_max = kd > sep_max ? kd : sep_max;
      sep2 = sep2 + d2;
    }
    uint64_t acc[kAcc] = {sum_bits(wx), sum_bits(wy), sum_bits(wvx), sum_bits(wvy), sum_bits(wv2), sum_bits(sep2), sum_bits(mass),
                          (uint64_t)min_x, (uint64_t)min_y, (uint64_t)max_x, (uint64_t)max_y, (uint64_t)speed, (uint64_t)sep_max,
                          counted, in_bounds, sep_rows};
    // stride 128
    if (l >= 128) {
#pragma unroll
      for (int f = 0; f < kAcc; ++f) upper[f][l - 128] = acc[f];
    }
    __syncthreads();
    if (l < 128) {
#pragma unroll
      for (int f = 0; f < kAcc; ++f) acc[f] = summary_join(f, acc[f], upper[f][l]);
    }
    // stride 64 (`second` is a buffer of its own: wave 0 may still be reading `upper`)
    if (l >= 64 && l < 128) {
#pragma unroll
      for (int f = 0; f < kAcc; ++f) second[f][l - 64] = acc[f];
    }
    __syncthreads();
    if (l < 64) {
#pragma unroll
      for (int f = 0; f < kAcc; ++f) acc[f] = summary_join(f, acc[f], second[f][l]);
      // strides 32 .. 1 within wave 0
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int f = 0; f < kAcc; ++f) acc[f] = summary_join(f, acc[f], (uint64_t)__shfl_xor((long long)acc[f], d, 64));
      }
      if (l == 0) {
        nbody_world_summary out;
        out.rows = s.n;
        out.counted = (int64_t)acc[kCounted];
        out.in_bounds = (int64_t)acc[kInBounds];
        out.sep_rows = (int64_t)acc[kSepRows];
        out.mass = sum_real(acc[kMass]);
        out.min_x = summary_unkey((int64_t)acc[kMinX]); out.min_y = summary_unkey((int64_t)acc[kMinY]);
        out.max_x = summary_unkey((int64_t)acc[kMaxX]); out.max_y = summary_unkey((int64_t)acc[kMaxY]);
        out.max_speed2 = summary_unkey((int64_t)acc[kSpeed]);
        out.sum_wx = sum_real(acc[kWx]); out.sum_wy = sum_real(acc[kWy]);
        out.sum_wvx = sum_real(acc[kWvx]); out.sum_wvy = sum_real(acc[kWvy]);
        out.sum_wv2 = sum_real(acc[kWv2]);
        out.sep_max2 = summary_unkey((int64_t)acc[kSepMax]);
        out.sep_sum2 = sum_real(acc[kSep2]);
        dst[summary_first_chunk(a, s.world) + s.chunk] = out;
      }
    }
    // (the next item's writes to `upper` come after its lanes 128 .. 255 passed the second barrier above, when every read of
    // `upper` was done; its writes to `second` come after its first barrier, which wave 0 reaches only when it is done here)
  }
}

// Field f (its index among the 17 of the record) of a world: its chunk records joined in ascending order.
__global__ __launch_bounds__(kSummaryBlock) void ensemble_summary_combine(const SummaryArgs a, const nbody_world_summary* __restrict__ chunks,
                                                                          nbody_world_summary* __restrict__ out) {
  const uint64_t idx = (uint64_t)blockIdx.x * kSummaryBlock + threadIdx.x;
  const uint32_t world = (uint32_t)(idx / kSummaryFields), f = (uint32_t)(idx - (uint64_t)world * kSummaryFields);
  if (world >= a.n_worlds) return;
  size_t row0;
  uint32_t n;
  summary_rows(a, world, row0, n);
  const uint32_t n_chunks = summary_chunks(n);
  const uint64_t* const src = reinterpret_cast<const uint64_t*>(chunks + summary_first_chunk(a, world)) + f;
  uint64_t v = src[0];  // (`rows`, field 0, is the segment's in every chunk record)
  for (uint32_t c = 1; c < n_chunks; ++c) {
    const uint64_t o = src[(size_t)c * kSummaryFields];
    if (f >= 1 && f <= 3) {
      v += o;  // counted, in_bounds, sep_rows
    } else if (f == 4 || (f >= 10 && f <= 14) || f == 16) {
      v = sum_bits(sum_real(v) + sum_real(o));  // mass (exact) and the ordered sums: chunk 0's value plus chunk 1's and so on
    } else if (f == 5 || f == 6) {
      v = summary_key(sum_real(o)) < summary_key(sum_real(v)) ? o : v;  // min_x, min_y
    } else if (f != 0) {
      v = summary_key(sum_real(o)) > summary_key(sum_real(v)) ? o : v;  // max_x, max_y, max_speed2, sep_max2
    }
  }
  reinterpret_cast<uint64_t*>(out + world)[f] = v;
}

}  // namespace

template <class T>
hipError_t launch_ensemble_summary(hipStream_t s, SummaryArgs a, int64_t n_chunks, nbody_world_summary* scratch, nbody_world_summary* out) {
  if (a.n_worlds < 1 || (int64_t)a.n_worlds > (1ll << 26) || !out || !a.pos || !a.vel || !a.mass || a.height > kSummaryMaxHeight ||
      (a.tpos && !a.tvel) || n_chunks < (int64_t)a.n_worlds || n_chunks > (1ll << 27))
    return hipErrorInvalidValue;
  if (a.table) {
    a.chunks = 0;
    if (!a.tracers) a.chunk_base = nullptr;
    if ((a.tracers && !a.chunk_base) || (!a.tracers && n_chunks != (int64_t)a.n_worlds)) return hipErrorInvalidValue;
  } else {
    const uint32_t n = a.tracers ? a.n_tracers : a.n_bodies;
    a.chunk_base = nullptr;
    a.chunks = summary_chunks(n);
    if ((uint64_t)n * a.n_worlds > (1ull << 26) || n_chunks != (int64_t)a.n_worlds * a.chunks) return hipErrorInvalidValue;
    if (a.tracers && n && !a.tpos) return hipErrorInvalidValue;
  }
  const bool several = n_chunks > (int64_t)a.n_worlds;
  if (several && !scratch) return hipErrorInvalidValue;
  const unsigned grid = (unsigned)(n_chunks < (int64_t)kSummaryMaxGrid ? n_chunks : (int64_t)kSummaryMaxGrid);
  hipLaunchKernelGGL(ensemble_summary_chunks<T>, dim3(grid), dim3(kSummaryBlock), 0, s, a, (uint64_t)n_chunks, several ? scratch : out);
  if (several) {
    const uint64_t lanes = (uint64_t)a.n_worlds * kSummaryFields;  // <= 2^26 * 17
    hipLaunchKernelGGL(ensemble_summary_combine, dim3((unsigned)((lanes + kSummaryBlock - 1) / kSummaryBlock)), dim3(kSummaryBlock), 0, s, a,
                       (const nbody_world_summary*)scratch, out);
  }
  return hipGetLastError();
}

template hipError_t launch_ensemble_summary<float>(hipStream_t, SummaryArgs, int64_t, nbody_world_summary*, nbody_world_summary*);
template hipError_t launch_ensemble_summary<double>(hipStream_t, SummaryArgs, int64_t, nbody_world_summary*, nbody_world_summary*);

}  // namespace nbody

using namespace nbody;

// The contract in host code: no device, no handle.
template <class T>
static int summary_of_checked(int64_t rows, const T* pos, const T* vel, const uint32_t* weight, const T* ref_pos, const T* ref_vel,
                              uint32_t height, nbody_world_summary* out) {
  if (rows < 0 || !out) return NBODY_ERR_INVALID;
  if (rows > 0 && (!pos || !vel)) return NBODY_ERR_INVALID;
  if (ref_pos && !ref_vel) return NBODY_ERR_INVALID;
  summary_of<T>(rows, pos, vel, weight, ref_pos, ref_vel, height, out);
  return NBODY_OK;
}

NB_API int nbody_summary_of_f32(int64_t rows, const float* pos_xy, const float* vel_xy, const uint32_t* weight, const float* ref_pos_xy,
                                const float* ref_vel_xy, uint32_t height, nbody_world_summary* out) {
  return summary_of_checked<float>(rows, pos_xy, vel_xy, weight, ref_pos_xy, ref_vel_xy, height, out);
}
NB_API int nbody_summary_of_f64(int64_t rows, const double* pos_xy, const double* vel_xy, const uint32_t* weight, const double* ref_pos_xy,
                                const double* ref_vel_xy, uint32_t height, nbody_world_summary* out) {
  return summary_of_checked<double>(rows, pos_xy, vel_xy, weight, ref_pos_xy, ref_vel_xy, height, out);
}
