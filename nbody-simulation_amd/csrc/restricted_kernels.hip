// Restricted ensembles: the tracers' step, worlds x tracer tiles in one launch (restricted_kernels.h).
//
// What every tracer computes:
//   a_t = sum_j calculate_gravity(p_t, p_j, w_j) over the bodies of its own world, j ascending      src/main.rs:234-253
//   v_t += a_t*dt ; x_t += v_t*dt                                                                   src/main.rs:419-423
// with no mass and no self term: a tracer on a body meets that body's pair like any other (EXACT's is_normal skip drops it, FAST
// adds exactly 0 through the biased denominator).
// The staging, the EXACT chain and the FAST sum are ensemble_world.h's, the text the bodies' kernel runs; a lane carries R tracers
// through them, R rows of 256 apart (coalesced), each with its own accumulators — a tracer's order of additions does not know R.
// Lanes past the end of a world's tracers compute a tracer at (0, 0) and store nothing.
// The block's body is rst_world_tile (restricted_device.h), shared with the ragged restricted kernel of rr_kernels.hip: this
// kernel only says which world and which tile a block is.
//
// This translation unit is compiled with -ffp-contract=off: nothing fuses unless written as an fma.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nbody_hip.h"
#include "restricted_device.h"
#include "restricted_kernels.h"

namespace nbody {
namespace {

// SWEEP (nbody_sweep_*): the world's own delta, clamp and route from its entry (ens_sweep_args); the tracers are updated in place, so
// the blocks of a world that has taken its steps return at once, before the staging and its barrier.
// (Left to itself the sweep's instantiation is scheduled into 100 VGPRs, 4 waves per SIMD, from the same instructions that take 58
// in the plain one: it is told to stay at 8 waves, and does without scratch.  The plain instantiation's bound is the default.)
template <int R, bool SWEEP>
__global__ __launch_bounds__(kEnsembleBlock) __attribute__((amdgpu_waves_per_eu(SWEEP ? 8 : 1))) void restricted_tracers(const EnsembleArgs b0, const RestrictedArgs t) {
  const unsigned world = blockIdx.x / t.tiles, tile = blockIdx.x - world * t.tiles;
  EnsembleArgs b = b0;
  if constexpr (SWEEP) {
    if (!ens_sweep_args(b, world)) return;
  }
  const int n = b.n_bodies;
  constexpr int64_t per_block = (int64_t)kEnsembleBlock * R;
  const int64_t first = (int64_t)tile * per_block;  // the tile's first tracer among its world's
  const int64_t left = t.n_tracers - first;
  TracerRows rows;
  rows.tpos = t.tpos, rows.tvel = t.tvel, rows.tacc_out = t.tacc_out;
  rst_world_tile<R>(b, rows, n, (size_t)world * (size_t)n, (size_t)world * (size_t)t.n_tracers + (size_t)first,
                    (int)(left < per_block ? left : per_block));
}

}  // namespace

hipError_t launch_restricted_tracers(hipStream_t s, int64_t n_worlds, const EnsembleArgs& bodies, RestrictedArgs t) {
  if (n_worlds < 1 || bodies.n_bodies < 1 || bodies.n_bodies > kEnsembleMaxBodies || n_worlds * bodies.n_bodies > kEnsembleMaxRows ||
      t.n_tracers < 1 || n_worlds > kEnsembleMaxRows / t.n_tracers || !t.tpos || !bodies.pos_in || !bodies.mass)
    return hipErrorInvalidValue;
  constexpr int64_t per_block = (int64_t)kEnsembleBlock * kRestrictedPerLane;
  t.tiles = (unsigned)((t.n_tracers + per_block - 1) / per_block);
  const dim3 grid((unsigned)(n_worlds * t.tiles));  // <= 2^26 blocks: n_worlds * n_tracers <= 2^26
  if (bodies.sweep) {
    if (!t.tvel) return hipErrorInvalidValue;  // (a sweep is a step)
    hipLaunchKernelGGL((restricted_tracers<kRestrictedPerLane, true>), grid, dim3(kEnsembleBlock), ensemble_lds_bytes(bodies.n_bodies), s, bodies, t);
  } else {
    hipLaunchKernelGGL((restricted_tracers<kRestrictedPerLane, false>), grid, dim3(kEnsembleBlock), ensemble_lds_bytes(bodies.n_bodies), s, bodies, t);
  }
  return hipGetLastError();
}

}  // namespace nbody
