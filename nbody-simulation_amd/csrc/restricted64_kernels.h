// Restricted ensembles in f64 (nbody_restricted64_*): the tracers' kernel.  Internal.
//
// The bodies of a restricted ensemble are stepped by launch_ensemble64_step (ensemble64_kernels.h), unchanged.  This launch steps
// the tracers: massless points, m per world, in the field of their own world's bodies at the positions that step's bodies launch
// reads.  The grid runs over worlds x tracer tiles; every block stages its world's bodies whole in LDS in the f64 ensemble's
// layout (ensemble64_lds_bytes(n) of dynamic LDS and NO static LDS: two blocks of 81 920 B are the CU's 160 KiB to the byte,
// ensemble64_world.h) and every lane owns kRestricted64PerLane tracers, which it alone reads and writes: they are updated in place.
//   EXACT  one lane per tracer: the terms of a block of kEns64TermBlock bodies (pair_term_select, two IEEE divisions), then added
//          in ascending row order — one chain of IEEE additions per tracer — then main.rs:419-423, multiply then add.  arith EXACT
//          and AUTO run it, as they do for the bodies and for an f64 context.
//   FAST   (opt-in: arith FAST with a clamp > 0) ONE LANE PER TRACER, whatever n is: the order of additions is
//          ens64_fast_sum<1> — the order the f64 ensemble's bodies have for n > 128 — a function of n alone.  The sources are NOT
//          split over lanes where a world has few tracers: a tracer's bits would then depend on m.
//   Route  the staging's OR of outside_fast(double) over the bodies is the world's decision, the same in every block of the world
//          and the same the bodies' blocks take: no flag buffer.  In a FAST world a tracer whose own pre-step position is outside
//          FAST's domain takes its EXACT value, computed alone after the FAST sum; its neighbours keep their FAST bits.
// A tracer's bits depend on its own state, its world's bodies, n and the params — not on m, its slot, the number of tracers per
// lane, the number of worlds, its world's index or the other worlds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ensemble64_kernels.h"

namespace nbody {

constexpr int kRestricted64PerLane = 2;  // tracers per lane (the table of 1 against 2; no scratch at 114 VGPRs)

struct Restricted64Args {
  double2* tpos = nullptr;      // [n_worlds][n_tracers], read and (with tvel) written by their own lane only
  double2* tvel = nullptr;      // updated in place; NULL: force only, tpos is not written
  double2* tacc_out = nullptr;  // or NULL
  int64_t n_tracers = 0;        // per world
  unsigned tiles = 1;           // blocks per world
};

// One step (or, without tvel, one force evaluation) of the tracers of all n_worlds worlds on `s`.  Of `bodies` pos_in, weight,
// n_bodies, delta, clamp and fast are read: what the bodies' launch of the same step is given.  A launch that cannot be made
// comes back as hipErrorInvalidValue.
// With bodies.sweep (a sweep's launch: tvel is required) world k's delta, clamp and route are its entry's, and its blocks return at
// once when bodies.step >= its steps (ens_sweep_args / ens64_sweep_args).
hipError_t launch_restricted64_tracers(hipStream_t s, int64_t n_worlds, const Ensemble64Args& bodies, Restricted64Args t);

}  // namespace nbody
