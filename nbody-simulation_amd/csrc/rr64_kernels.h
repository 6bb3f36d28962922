// Ragged restricted ensembles in f64 (nbody_rr64_*): the tracers' kernel over work items.  Internal.
//
// The bodies of a ragged restricted ensemble are stepped by launch_ensemble64_step_ragged (ensemble64_kernels.h), unchanged.
// This launch steps the tracers of worlds that differ in size and in their number of tracers.  A block is one 16-byte work item
// of the table that rr_plan.h lays out under ensemble64_lds_bytes: {body_row0, n, tracer_row0, count} — the first of the world's
// body rows among all body rows, its size, the first of the tile's tracer rows among all tracer rows, and the tracers of the
// tile, 1 .. 512 (kEnsembleBlock * kRestricted64PerLane).  What a block computes is rst64_world_tile (restricted64_device.h), the
// text the uniform kernel of restricted64_kernels.hip runs: EXACT (arith EXACT and AUTO), FAST (opt-in; one lane per tracer, the
// order of additions a function of n alone) and the route (per world and per step from the staging's OR, with the per-tracer
// exception) are stated in restricted64_kernels.h, and a tracer's bits are those of nbody_restricted64_* holding its world alone.
// No static LDS: two blocks of 81 920 B are the CU's 160 KiB to the byte.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ensemble64_kernels.h"
#include "restricted64_kernels.h"  // kRestricted64PerLane

namespace nbody {

struct Rr64TracerArgs {
  double2* tpos = nullptr;      // the tracer rows of all worlds, world after world; read and (with tvel) written by their own lane only
  double2* tvel = nullptr;      // updated in place; NULL: force only, tpos is not written
  double2* tacc_out = nullptr;  // or NULL
};

// One launch of the tracers' plan on `s`: `blocks` work items from `items`, `lds_bytes` = ensemble64_lds_bytes of the largest
// world among them (above 64 KB this kernel's own dynamic-LDS limit is raised, once per device).  Of `bodies` pos_in, weight,
// delta, clamp and fast are read: what the bodies' launches of the same step are given.
// Refused: blocks < 1 or > 2^26, a NULL table or NULL arrays, lds_bytes above ensemble64_lds_bytes(4096).
// With bodies.sweep (a sweep's launch: tvel is required) world k's delta, clamp and route are its entry's, and its blocks return at
// once when bodies.step >= its steps (ens_sweep_args / ens64_sweep_args); the world of every item comes from bodies.item_world.
hipError_t launch_rr64_tracers(hipStream_t s, int64_t blocks, size_t lds_bytes, const uint4* items, const Ensemble64Args& bodies,
                               const Rr64TracerArgs& t);

}  // namespace nbody
