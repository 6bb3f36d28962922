// Restricted ensembles in f64: the tracers' step, worlds x tracer tiles in one launch (restricted64_kernels.h).
//
// What every tracer computes, in double:
//   a_t = sum_j calculate_gravity(p_t, p_j, w_j as f64) over the bodies of its own world, j ascending      src/main.rs:234-253
//   v_t += a_t*dt ; x_t += v_t*dt                                                                          src/main.rs:419-423
// with no mass and no self term: a tracer on a body meets that body's pair like any other (EXACT's is_normal skip drops it, FAST
// adds exactly 0 through the biased denominator).
// The staging, the EXACT chain and the FAST sum are ensemble64_world.h's, the text the bodies' kernel runs; a lane carries R
// tracers through them, R rows of 256 apart (coalesced), each with its own accumulators — a tracer's order of additions does not
// know R.  Lanes past the end of a world's tracers compute a tracer at (0, 0) and store nothing.  No static LDS.
// The block's body is rst64_world_tile (restricted64_device.h), shared with the ragged restricted kernel of rr64_kernels.hip: this
// kernel only says which world and which tile a block is.
//
// This translation unit is compiled with -ffp-contract=off: nothing fuses unless written as an fma.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nbody_hip.h"
#include "restricted64_device.h"
#include "restricted64_kernels.h"

namespace nbody {
namespace {

// SWEEP (nbody_sweep_*): the world's own delta, clamp and route from its entry (ens64_sweep_args); the tracers are updated in place, so
// the blocks of a world that has taken its steps return at once, before the staging and its barrier.
template <int R, bool SWEEP>
__global__ __launch_bounds__(kEnsembleBlock) void restricted64_tracers(const Ensemble64Args b0, const Restricted64Args t) {
  const unsigned world = blockIdx.x / t.tiles, tile = blockIdx.x - world * t.tiles;
  Ensemble64Args b = b0;
  if constexpr (SWEEP) {
    if (!ens64_sweep_args(b, world)) return;
  }
  const int n = b.n_bodies;
  constexpr int64_t per_block = (int64_t)kEnsembleBlock * R;
  const int64_t first = (int64_t)tile * per_block;  // the tile's first tracer among its world's
  const int64_t left = t.n_tracers - first;
  Tracer64Rows rows;
  rows.tpos = t.tpos, rows.tvel = t.tvel, rows.tacc_out = t.tacc_out;
  rst64_world_tile<R>(b, rows, n, (size_t)world * (size_t)n, (size_t)world * (size_t)t.n_tracers + (size_t)first,
                      (int)(left < per_block ? left : per_block));
}

}  // namespace

hipError_t launch_restricted64_tracers(hipStream_t s, int64_t n_worlds, const Ensemble64Args& bodies, Restricted64Args t) {
  if (n_worlds < 1 || bodies.n_bodies < 1 || bodies.n_bodies > kEnsembleMaxBodies || n_worlds * bodies.n_bodies > kEnsembleMaxRows ||
      t.n_tracers < 1 || n_worlds > kEnsembleMaxRows / t.n_tracers || !t.tpos || !bodies.pos_in || !bodies.weight)
    return hipErrorInvalidValue;
  constexpr int64_t per_block = (int64_t)kEnsembleBlock * kRestricted64PerLane;
  t.tiles = (unsigned)((t.n_tracers + per_block - 1) / per_block);
  const dim3 grid((unsigned)(n_worlds * t.tiles));  // <= 2^26 blocks: n_worlds * n_tracers <= 2^26
  const size_t lds = ensemble64_lds_bytes(bodies.n_bodies);
  if (lds > 65536) {  // its own function, so its own limit: the bodies' kernels' raised ones do not cover it
    static std::atomic<bool> raised[64], raised_sweep[64];
    const hipError_t h =
        bodies.sweep ? ens64_raise_lds_limit(reinterpret_cast<const void*>(&restricted64_tracers<kRestricted64PerLane, true>), raised_sweep)
                     : ens64_raise_lds_limit(reinterpret_cast<const void*>(&restricted64_tracers<kRestricted64PerLane, false>), raised);
    if (h != hipSuccess) return h;
  }
  if (bodies.sweep) {
    if (!t.tvel) return hipErrorInvalidValue;  // (a sweep is a step)
    hipLaunchKernelGGL((restricted64_tracers<kRestricted64PerLane, true>), grid, dim3(kEnsembleBlock), lds, s, bodies, t);
  } else {
    hipLaunchKernelGGL((restricted64_tracers<kRestricted64PerLane, false>), grid, dim3(kEnsembleBlock), lds, s, bodies, t);
  }
  return hipGetLastError();
}

}  // namespace nbody
