// Summaries of an ensemble (nbody_summary_*): one nbody_world_summary per world from one call, for all eight ensemble handles,
// and the pure-host restatement behind nbody_summary_of_f32 / _of_f64.  Internal.  A segment is one world's bodies or one world's
// tracers; its record is a function of its own rows (and of the reference world's rows, for the separation) and of nothing else.
//
// Arithmetic.  Everything is double.  x, y, vx, vy are widened (exact); w is the double of what the handle holds (`weight as
// f32` on the f32 handles, the u32 weight on the f64 ones, 1 for a tracer).  Every *, + and - is one IEEE double operation in
// the grouping written in summary_of below; nothing is contracted (the library is built with -ffp-contract=off).
//
// Order.  mass is a sum of integers below 2^53: exact, so order-free.  The minima, maxima, max_speed2 and sep_max2 are ordered by
// value with -0.0 below +0.0 (summary_key): order-free.  The six ordered sums (sum_wx, sum_wy, sum_wvx, sum_wvy, sum_wv2,
// sep_sum2) are added in an order that is a function of the row index alone:
//   a segment is cut into chunks of kSummaryChunk = 4096 rows;
//   in chunk c, chain l (0 <= l < 256) starts at +0.0 and adds the terms of rows 4096 c + l + 256 i, i = 0 .. 15 ascending (a row
//     past the end, or one that does not contribute, adds nothing);
//   then for s = 128, 64, .., 1: P[l] = P[l] + P[l + s] for l < s; the chunk's value is P[0];
//   the segment's value is chunk 0's value plus chunk 1's and so on, ascending.
// summary_of below is that sentence in host code; the kernel (ensemble_summary.hip) is one 256-thread block per (world, chunk):
// lane l is chain l, strides 128 and 64 go through LDS, strides 32 .. 1 through lane shuffles in wave 0.  A second small launch
// adds the chunks of every world in ascending order where a segment has more than one (tracers only: bodies are one chunk).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <limits>

#include "../../include/nbody_hip.h"
#include "ensemble_rows.h"

namespace nbody {

constexpr int kSummaryBlock = 256;                  // chains per chunk: one lane each
constexpr int kSummaryPerLane = 16;                 // rows per chain
constexpr int64_t kSummaryChunk = kSummaryBlock * kSummaryPerLane;  // 4096 rows
constexpr uint32_t kSummaryMaxHeight = 1u << 24;    // as the frames': `height as f32` exact
constexpr int kSummaryFields = 17;                  // 8-byte fields of nbody_world_summary
static_assert(sizeof(nbody_world_summary) == 8 * kSummaryFields, "17 fields of 8 bytes, no padding");

// The chunks of a segment of n rows; a segment without rows is one chunk that adds nothing.
__host__ __device__ inline uint32_t summary_chunks(uint32_t n) { return n ? (n + (uint32_t)kSummaryChunk - 1) / (uint32_t)kSummaryChunk : 1u; }

// A double as an integer that orders as the value does, -0.0 below +0.0 (never given a NaN: only finite rows enter, and a
// square or a sum of squares of finite values is +inf at the worst).
__host__ __device__ inline int64_t summary_key(double v) {
  const int64_t b = __builtin_bit_cast(int64_t, v);
  return b ^ ((b >> 63) & 0x7fffffffffffffffll);
}
__host__ __device__ inline double summary_unkey(int64_t k) {
  return __builtin_bit_cast(double, k ^ ((k >> 63) & 0x7fffffffffffffffll));
}

__host__ __device__ inline bool summary_finite(double v) { return v - v == 0.0; }  // (inf - inf and NaN - NaN are NaN)

struct SummaryArgs {
  const void* pos = nullptr;    // T2 rows of all worlds (the handle's current buffer)
  const void* vel = nullptr;
  const void* mass = nullptr;   // float rows (T = float) or uint32_t rows (T = double)
  const void* tpos = nullptr;   // tracers (may be NULL where no world has one)
  const void* tvel = nullptr;
  const WorldRanges* table = nullptr;      // ragged: one per world (device); NULL: uniform
  const uint32_t* chunk_base = nullptr;   // ragged, tracers: [n_worlds + 1], the first chunk of every world's tracers and the total
  const int32_t* ref = nullptr;           // [n_worlds] (device) or NULL: no separation
  uint32_t n_bodies = 0, n_tracers = 0;   // uniform: per world
  uint32_t n_worlds = 0;
  uint32_t chunks = 0;          // uniform: the chunks of every world's segment (set by the launch)
  uint32_t height = 0;
  uint32_t tracers = 0;         // the tracers' segments, not the bodies'
};

// All worlds' records on `s`: out[n_worlds] (device).  n_chunks: the chunks of all addressed segments together (n_worlds where
// every segment is one chunk); where it is more, `scratch` holds n_chunks records (device) and a second launch adds them up.
// Arguments that do not fit come back as hipErrorInvalidValue, never as a launch.
template <class T>
hipError_t launch_ensemble_summary(hipStream_t s, SummaryArgs a, int64_t n_chunks, nbody_world_summary* scratch, nbody_world_summary* out);

// ---- the host restatement: one segment's record by the contract above.  ref_pos == NULL: no separation.
template <class T>
void summary_of(int64_t rows, const T* pos, const T* vel, const uint32_t* weight, const T* ref_pos, const T* ref_vel, uint32_t height,
                nbody_world_summary* out) {
  const double inf = std::numeric_limits<double>::infinity();
  nbody_world_summary r{};
  r.rows = rows;
  int64_t kmin_x = summary_key(inf), kmin_y = kmin_x, kmax_x = summary_key(-inf), kmax_y = kmax_x, kspeed = summary_key(0.0), ksep = kspeed;
  const double h = (double)height;
  for (int64_t c0 = 0; c0 < rows || c0 == 0; c0 += kSummaryChunk) {
    double P[6][kSummaryBlock];
    for (auto& f : P)
      for (double& v : f) v = 0.0;
    for (int l = 0; l < kSummaryBlock; ++l)
      for (int i = 0; i < kSummaryPerLane; ++i) {
        const int64_t row = c0 + l + (int64_t)kSummaryBlock * i;
        if (row >= rows) break;
        const double x = (double)pos[2 * row], y = (double)pos[2 * row + 1], vx = (double)vel[2 * row], vy = (double)vel[2 * row + 1];
        if (y < h && x < h && y >= 0.0 && x >= 0.0) ++r.in_bounds;
        if (!(summary_finite(x) && summary_finite(y) && summary_finite(vx) && summary_finite(vy))) continue;
        const double w = weight ? (sizeof(T) == 4 ? (double)(float)weight[row] : (double)weight[row]) : 1.0;
        const double v2 = vx * vx + vy * vy;
        ++r.counted;
        r.mass += w;
        kmin_x = std::min(kmin_x, summary_key(x)); kmax_x = std::max(kmax_x, summary_key(x));
        kmin_y = std::min(kmin_y, summary_key(y)); kmax_y = std::max(kmax_y, summary_key(y));
        kspeed = std::max(kspeed, summary_key(v2));
        P[0][l] = P[0][l] + w * x;
        P[1][l] = P[1][l] + w * y;
        P[2][l] = P[2][l] + w * vx;
        P[3][l] = P[3][l] + w * vy;
        P[4][l] = P[4][l] + w * v2;
        if (!ref_pos) continue;
        const double rx = (double)ref_pos[2 * row], ry = (double)ref_pos[2 * row + 1];
        if (!(summary_finite(rx) && summary_finite(ry) && summary_finite((double)ref_vel[2 * row]) && summary_finite((double)ref_vel[2 * row + 1])))
          continue;
        const double dx = x - rx, dy = y - ry, d2 = dx * dx + dy * dy;
        ++r.sep_rows;
        ksep = std::max(ksep, summary_key(d2));
        P[5][l] = P[5][l] + d2;
      }
    for (int s = kSummaryBlock / 2; s >= 1; s /= 2)
      for (auto& f : P)
        for (int l = 0; l < s; ++l) f[l] = f[l] + f[l + s];
    double* const sums[6] = {&r.sum_wx, &r.sum_wy, &r.sum_wvx, &r.sum_wvy, &r.sum_wv2, &r.sep_sum2};
    for (int f = 0; f < 6; ++f) *sums[f] = c0 == 0 ? P[f][0] : *sums[f] + P[f][0];
  }
  r.min_x = summary_unkey(kmin_x); r.min_y = summary_unkey(kmin_y);
  r.max_x = summary_unkey(kmax_x); r.max_y = summary_unkey(kmax_y);
  r.max_speed2 = summary_unkey(kspeed);
  r.sep_max2 = summary_unkey(ksep);
  *out = r;
}

}  // namespace nbody
