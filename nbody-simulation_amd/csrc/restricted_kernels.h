// Restricted ensembles (nbody_restricted_*): the tracers' kernel.  Internal.
//
// The bodies of a restricted ensemble are stepped by launch_ensemble_step (ensemble_kernels.h), unchanged.  This launch steps the
// tracers: massless points, m per world, in the field of their own world's bodies at the positions that step's bodies launch
// reads.  The grid runs over worlds x tracer tiles; every block stages its world's bodies whole in LDS in the ensemble's couple
// layout (ensemble_lds_bytes(n) of dynamic LDS, ensemble_world.h) and every lane owns kRestrictedPerLane tracers, which it alone
// reads and writes: they are updated in place.
//   EXACT  one ascending-row chain of pair_as_written<float> per tracer, then main.rs:419-423, multiply then add.
//   FAST   ONE LANE PER TRACER, whatever n is: the order of additions is ens_fast_sum<1> — the order the ensemble's bodies have
//          for n > 128 — a function of n alone.  The sources are NOT split over lanes where a world has few tracers: a tracer's
//          bits would then depend on m.  A shape with few tracers per world leaves lanes idle; that is the price of the promise.
//   AUTO   the block-wide OR of outside_fast() over the bodies it stages is the world's decision, the same in every block of the
//          world and the same the bodies' blocks take: no flag buffer.  In a FAST world a tracer whose own pre-step position is
//          outside FAST's domain takes its EXACT value; its neighbours keep their FAST bits.
// A tracer's bits depend on its own state, its world's bodies, n and the params — not on m, its slot, the number of worlds, its
// world's index or the other worlds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ensemble_kernels.h"

namespace nbody {

constexpr int kRestrictedPerLane = 2;  // tracers per lane: every couple read from LDS feeds 2 * kRestrictedPerLane pairs

struct RestrictedArgs {
  float2* tpos = nullptr;     // [n_worlds][n_tracers], read and (with tvel) written by their own lane only
  float2* tvel = nullptr;     // updated in place; NULL: force only, tpos is not written
  float2* tacc_out = nullptr; // or NULL
  int64_t n_tracers = 0;      // per world
  unsigned tiles = 1;         // blocks per world
};

// One step (or, without tvel, one force evaluation) of the tracers of all n_worlds worlds on `s`.  Of `bodies` pos_in, mass,
// n_bodies, delta, clamp and arith are read: what the bodies' launch of the same step is given.
// With bodies.sweep (a sweep's launch: tvel is required) world k's delta, clamp and route are its entry's, and its blocks return at
// once when bodies.step >= its steps (ens_sweep_args / ens64_sweep_args).
hipError_t launch_restricted_tracers(hipStream_t s, int64_t n_worlds, const EnsembleArgs& bodies, RestrictedArgs t);

}  // namespace nbody
