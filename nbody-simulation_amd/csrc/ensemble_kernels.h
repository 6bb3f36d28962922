// Ensembles (nbody_ensemble_*): many small worlds of equal size stepped by ONE launch per step.  Internal.
//
// A world's sources (<= 4096 bodies: 48 KB as position couples + masses) fit in LDS, so the grid runs over worlds x target
// tiles: every block stages its world's sources once, takes the FAST / EXACT decision of AUTO while it loads them, and
// computes one tile of that world's targets.  Layouts, per size range (ensemble_split):
//   n > 128        one target per lane, 256 targets per block, ceil(n / 256) blocks per world;
//   n <= 128       one block per world; the sources of a target are split over SPLIT = 256 / pow2ceil(n) consecutive lanes
//                  (2 .. 64, at least 4 targets per block) and their partial sums meet in a butterfly of DPP adds inside a
//                  row of 16 lanes, v_permlane16_swap across rows, v_permlane32_swap across the halves of the wave.
// FAST's order of additions is a function of n alone (ensemble_kernels.hip), EXACT is one ascending-j chain per target.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nbody {

constexpr int kEnsembleMaxBodies = 4096;
constexpr int64_t kEnsembleMaxRows = 1ll << 26;  // n_worlds * n_bodies
constexpr int kEnsembleBlock = 256;

struct EnsembleArgs {
  const float2* pos_in = nullptr;  // [n_worlds][n_bodies], read by every block of the world
  const float* mass = nullptr;     // `weight as f32`
  float2* pos_out = nullptr;       // the other position buffer (NULL with vel: force only)
  float2* vel = nullptr;           // updated in place
  float2* acc_out = nullptr;       // or NULL
  int n_bodies = 0;
  unsigned tiles = 1;              // blocks per world
  float delta = 0.f, clamp = 0.f;
  int arith = 0;                   // nbody_arith; AUTO decides per world in the kernel
};

// Lanes that share one target's sources.
inline int ensemble_split(int n_bodies) {
  if (n_bodies > 128) return 1;
  int split = 2, targets = 128;
  while (targets / 2 >= n_bodies && split < 64) { targets /= 2; split *= 2; }
  return split;
}
inline size_t ensemble_lds_bytes(int n_bodies) { return (size_t)((n_bodies + 1) / 2) * 24; }  // couples {xA, xB, yA, yB} + {mA, mB}

// One step (or, without vel / pos_out, one force evaluation) of all n_worlds worlds on `s`.
hipError_t launch_ensemble_step(hipStream_t s, int64_t n_worlds, EnsembleArgs a);

}  // namespace nbody
