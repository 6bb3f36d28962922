// Ragged restricted ensembles (nbody_rr_*): the tracers' kernel over work items.  Internal.
//
// The bodies of a ragged restricted ensemble are stepped by launch_ensemble_step_ragged (ensemble_kernels.h), unchanged.  This
// launch steps the tracers of worlds that differ in size and in their number of tracers.  A block is one 16-byte work item of
// the table that rr_plan.h lays out: {body_row0, n, tracer_row0, count} — the first of the world's body rows among all body rows,
// its size, the first of the tile's tracer rows among all tracer rows, and the tracers of the tile, 1 .. 512 (kEnsembleBlock *
// kRestrictedPerLane).  What a block computes is rst_world_tile (restricted_device.h), the text the uniform kernel of
// restricted_kernels.hip runs: EXACT, FAST (one lane per tracer, the order of additions a function of n alone), AUTO (per world
// and per step from the staging block's OR, with the per-tracer exception) are stated there, and a tracer's bits are those of
// nbody_restricted_* holding its world alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ensemble_kernels.h"
#include "restricted_kernels.h"  // kRestrictedPerLane

namespace nbody {

struct RrTracerArgs {
  float2* tpos = nullptr;      // the tracer rows of all worlds, world after world; read and (with tvel) written by their own lane only
  float2* tvel = nullptr;      // updated in place; NULL: force only, tpos is not written
  float2* tacc_out = nullptr;  // or NULL
};

// One launch of the tracers' plan on `s`: `blocks` work items from `items`, `lds_bytes` = ensemble_lds_bytes of the largest world
// among them.  Of `bodies` pos_in, mass, delta, clamp and arith are read: what the bodies' launches of the same step are given.
// Refused: blocks < 1 or > 2^26, a NULL table or NULL arrays, lds_bytes above ensemble_lds_bytes(4096).
// With bodies.sweep (a sweep's launch: tvel is required) world k's delta, clamp and route are its entry's, and its blocks return at
// once when bodies.step >= its steps (ens_sweep_args / ens64_sweep_args); the world of every item comes from bodies.item_world.
hipError_t launch_rr_tracers(hipStream_t s, int64_t blocks, size_t lds_bytes, const uint4* items, const EnsembleArgs& bodies,
                             const RrTracerArgs& t);

}  // namespace nbody
