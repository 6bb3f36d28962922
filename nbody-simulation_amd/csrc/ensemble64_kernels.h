// Ensembles in f64 (nbody_ensemble64_*): many small double-precision worlds of equal size stepped by ONE launch per step;
// worlds of different sizes (nbody_ragged64_*) run the same block body from a table of work items: at the end.
// Internal.  The launch shape is that of ensemble_kernels.h — worlds x target tiles, every block stages its world's sources
// whole in LDS and takes FAST's per-world decision while it loads them — with these differences:
//   LDS      double2 positions and the u32 WEIGHTS (converted on use: `weight as f64` is exact, so the bits are those of a
//            double mass): 20 bytes a body, 81 920 B at n = 4096.  Two such blocks are 163 840 B, the CU's 160 KiB to the byte,
//            so the kernel may use NO static LDS (its block-wide OR borrows a staged word instead of __syncthreads_or's 256 B;
//            the compiler's resource remark must read "LDS Size [bytes/block]: 0").  With double masses a block would be 96 KB:
//            one block per CU, one wave per SIMD, for every n above 3408, under a kernel that waits on division chains.  That
//            two blocks of 81 920 B are in fact resident together is the arithmetic's claim, not a measured one.
//            Rows are padded to a multiple of the EXACT term block with NaN positions (a skipped pair: a -0.0 term).
//   arith    EXACT unless FAST is asked for by name with a clamp > 0 (driver.h, direct_fast_f64); FAST is gated per world and
//            per step on outside_fast(double).
//   layouts  ensemble_split's table: n > 128 one target per lane, ceil(n / 256) blocks per world; n <= 128 one block per world
//            and, under FAST, SPLIT = 256 / pow2ceil(n) lanes per target.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "ensemble_kernels.h"

namespace nbody {

// Sweeps (nbody_sweep_*) in f64: a world's own time step, clamp (the caller's float, widened) and number of steps.  One entry
// per world, 24 bytes, read once per block by scalar loads.
struct Ens64SweepWorld {
  double delta, clamp;
  int32_t steps, pad;
};

struct Ensemble64Args {
  const double2* pos_in = nullptr;   // [n_worlds][n_bodies], read by every block of the world
  const uint32_t* weight = nullptr;  // the mass is `weight as f64`
  double2* pos_out = nullptr;        // the other position buffer (NULL with vel: force only)
  double2* vel = nullptr;            // updated in place
  double2* acc_out = nullptr;        // or NULL
  int n_bodies = 0;
  unsigned tiles = 1;                // blocks per world
  double delta = 0.0, clamp = 0.0;
  int fast = 0;                      // FAST where the world's positions allow it; 0: every world EXACT
  // a sweep's launches only, as in EnsembleArgs
  const Ens64SweepWorld* sweep = nullptr;
  const uint32_t* item_world = nullptr;
  int step = 0;
};

// kEns64TermBlock, ensemble64_padded and ensemble64_lds_bytes come from ensemble_shape.h (plain C++: the ragged plan uses them).
static_assert(sizeof(double2) + sizeof(uint32_t) == 2 * sizeof(double) + sizeof(uint32_t), "a staged body is a double2 and a u32");

// One step (or, without vel / pos_out, one force evaluation) of all n_worlds worlds on `s`.  The limits are the f32 ensemble's
// (kEnsembleMaxBodies, kEnsembleMaxRows); a launch that cannot be made comes back as an error, never as an unlaunched step.
hipError_t launch_ensemble64_step(hipStream_t s, int64_t n_worlds, Ensemble64Args a);

// Ragged ensembles in f64 (nbody_ragged64_*): worlds of different sizes.  A block is one work item (world, tile) of the table
// that ragged_plan.h lays out, {row0, n | tile << 16}, as in launch_ensemble_step_ragged.  One launch of the plan: `blocks` items
// from `items`, `lds_bytes` = ensemble64_lds_bytes of the largest world among them (above 64 KB the ragged kernel's own
// dynamic-LDS limit is raised, once per device); n_bodies and tiles of `a` are not read.  Every world computes exactly what
// launch_ensemble64_step computes for a world of its size.
hipError_t launch_ensemble64_step_ragged(hipStream_t s, int64_t blocks, size_t lds_bytes, const uint2* items, Ensemble64Args a);

// Raises `kernel`'s limit of dynamic LDS to ensemble64_lds_bytes(kEnsembleMaxBodies), once per device: `raised` is that
// function's own zero-initialised table of 64 (a raised limit covers one function, so every kernel that stages a world of more
// than 64 KB keeps a table: the two above, and the tracers' kernels of restricted64_kernels.h and rr64_kernels.h).
hipError_t ens64_raise_lds_limit(const void* kernel, std::atomic<bool>* raised);

}  // namespace nbody
