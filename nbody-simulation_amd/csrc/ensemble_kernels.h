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
// Worlds of different sizes (nbody_ragged_*) run the same block body from a table of (world, tile) work items: below.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ensemble_shape.h"  // kEnsembleMaxBodies, kEnsembleMaxRows, kEnsembleBlock, ensemble_split, ensemble_lds_bytes

namespace nbody {

// Sweeps (nbody_sweep_*): what a world reads of its own where a call gives every world a time step, a clamp and a number of
// steps.  One entry per world, 16 bytes, read once per block by scalar loads (the world's index is the same in every lane).
struct EnsSweepWorld {
  float delta, clamp;
  int32_t steps, pad;
};

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
  // a sweep's launches only (the plain kernels read none of them): every world's entry, the step of the call that this
  // launch is, and — ragged launches — the world of every work item of this launch
  const EnsSweepWorld* sweep = nullptr;
  const uint32_t* item_world = nullptr;
  int step = 0;
};

// One step (or, without vel / pos_out, one force evaluation) of all n_worlds worlds on `s`.  With a.sweep the launch is a second
// instantiation of the same kernel (ensemble_kernels.hip, "Sweeps"): world k takes delta and clamp from its entry, turns EXACT
// where direct_arith_f32 would turn a handle with that clamp EXACT, and once a.step >= steps it only carries its positions over.
hipError_t launch_ensemble_step(hipStream_t s, int64_t n_worlds, EnsembleArgs a);

// Ragged ensembles (nbody_ragged_*): worlds of different sizes.  A block is one work item (world, tile) of the table that
// ragged_plan.h lays out: {row0, n | tile << 16} — the world's first row among all rows, its size, the tile of its targets.  One
// launch of the plan: `blocks` items from `items`, `lds_bytes` = ensemble_lds_bytes of the largest world among them; n_bodies and
// tiles of `a` are not read.  Every world computes exactly what launch_ensemble_step computes for a world of its size.
hipError_t launch_ensemble_step_ragged(hipStream_t s, int64_t blocks, size_t lds_bytes, const uint2* items, EnsembleArgs a);

}  // namespace nbody
