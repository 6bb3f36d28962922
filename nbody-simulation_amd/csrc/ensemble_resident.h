// Resident runs (nbody_resident_*): a sweep whose worlds stay in LDS for a whole launch.  Internal.
//
// A world of at most kResidentMaxBodies bodies is one block of the stepping kernels in both precisions (ensemble_split: n <= 128
// one block with its sources split over lanes, 129 .. 256 one tile of 256 targets), and that block reads nothing another block
// writes.  So one block per world stages its world once — positions and masses in the layout of ensemble_world.h /
// ensemble64_world.h, the velocities behind them — takes up to kResidentStepsPerLaunch of the world's steps of the call in a
// loop, and writes its rows back once, in place.  A step is the text the stepping kernels run (ens_exact_sum, ens_fast_sum,
// ens_group_sum, ens64_exact_sum, ens64_fast_sum) and the integration below is ens_integrate's expression, so every bit is the
// sweep's.  ensemble_resident.hip and ensemble64_resident.hip are the two kernels; ens_resident_with (ensemble_driver.h) is
// their host side.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ensemble64_kernels.h"
#include "ensemble_kernels.h"
#include "ensemble_shape.h"

namespace nbody {

constexpr int kResidentMaxBodies = 256;         // a world that is one block: tiles == 1 in both precisions
constexpr int kResidentStepsPerLaunch = 1024;   // a launch takes at most this many steps of the call

// The dynamic LDS of a world's block: the stepping kernels' layout and, behind it, the world's velocities.
inline size_t ensemble_resident_lds_bytes(int n_bodies) { return ensemble_lds_bytes(n_bodies) + (size_t)n_bodies * 2 * sizeof(float); }
inline size_t ensemble64_resident_lds_bytes(int n_bodies) { return ensemble64_lds_bytes(n_bodies) + (size_t)n_bodies * 2 * sizeof(double); }

// What nbody_resident_plan answers: the launches of a call and their dynamic LDS.  -> 0, or the index (from 1) of the argument
// it refuses: 1 n_worlds / n_bodies, 2 a size outside 1 .. kResidentMaxBodies, 3 n_steps, 4 a steps[k] outside 0 .. n_steps.
inline int resident_plan(int64_t n_worlds, const int64_t* n_bodies, const int32_t* steps, int n_steps, int is_f64, int32_t* n_launches,
                         int32_t* lds_bytes) {
  if (n_worlds < 1 || !n_bodies) return 1;
  if (n_steps < 0) return 3;
  int64_t largest = 0;
  int32_t most = steps ? 0 : n_steps;
  for (int64_t k = 0; k < n_worlds; ++k) {
    if (n_bodies[k] < 1 || n_bodies[k] > kResidentMaxBodies) return 2;
    if (n_bodies[k] > largest) largest = n_bodies[k];
    if (steps) {
      if (steps[k] < 0 || steps[k] > n_steps) return 4;
      if (steps[k] > most) most = steps[k];
    }
  }
  if (n_launches) *n_launches = (most + kResidentStepsPerLaunch - 1) / kResidentStepsPerLaunch;
  if (lds_bytes) *lds_bytes = (int32_t)(is_f64 ? ensemble64_resident_lds_bytes((int)largest) : ensemble_resident_lds_bytes((int)largest));
  return 0;
}

// One launch of a resident run on `s`: one block per world, a.sweep the table of the call, a.step the first step of the call
// that this launch takes; world k takes min(steps[k] - a.step, kResidentStepsPerLaunch) steps, or none.  a.pos_in is read and
// written in place, and so is a.vel; a.pos_out, a.tiles and a.item_world are not read.  worlds == NULL: every world has
// a.n_bodies rows; otherwise worlds[k] = {row0, n} and a.n_bodies is not read.  lds_bytes is that of the largest world.
hipError_t launch_ensemble_resident(hipStream_t s, int64_t n_worlds, const uint2* worlds, size_t lds_bytes, EnsembleArgs a);
hipError_t launch_ensemble64_resident(hipStream_t s, int64_t n_worlds, const uint2* worlds, size_t lds_bytes, Ensemble64Args a);

#if defined(__HIPCC__)
// main.rs:419-423 for the owner of a target, as ens_integrate (ensemble_device.h) writes it — multiply then add, no contraction
// (TU flag) — with the velocity from LDS and both results in registers: the stores wait for the step's barrier.
template <class T, class Vec2> __device__ __forceinline__ void ens_resident_integrate(const T delta, const T px, const T py, const T ax, const T ay,
                                                                                      Vec2& v, Vec2& x) {
  v.x = v.x + ax * delta;
  v.y = v.y + ay * delta;
  const T sx = v.x * delta, sy = v.y * delta;
  x = Vec2{px + sx, py + sy};
}
#endif

}  // namespace nbody
