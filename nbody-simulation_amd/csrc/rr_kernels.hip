// Ragged restricted ensembles: the tracers' step from a table of work items (rr_kernels.h).
//
// What every tracer computes is what restricted_kernels.hip states:
//   a_t = sum_j calculate_gravity(p_t, p_j, w_j) over the bodies of its own world, j ascending      src/main.rs:234-253
//   v_t += a_t*dt ; x_t += v_t*dt                                                                   src/main.rs:419-423
// and the block's body is the same text, rst_world_tile (restricted_device.h): this kernel only reads which world and which of
// its tracers a block is from its work item, where the uniform kernel computes them from blockIdx.
//
// This translation unit is compiled with -ffp-contract=off: nothing fuses unless written as an fma.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nbody_hip.h"
#include "restricted_device.h"
#include "rr_kernels.h"

namespace nbody {
namespace {

// The block's work item {body_row0, n, tracer_row0, count} is the same in every lane (a scalar load), so n and count are
// uniform: the barrier of the staging sees every thread.  Dynamic LDS is the launch's; the kernel uses no other.
// SWEEP (nbody_sweep_*): the item's world from b0.item_world, a table beside the items' (by the same kind of load), and with it
// the world's own delta, clamp and route (ens_sweep_args); the blocks of a world that has taken its steps return at once.
template <int R, bool SWEEP>
__global__ __launch_bounds__(kEnsembleBlock) void rr_tracers(const EnsembleArgs b0, const RrTracerArgs t, const uint4* __restrict__ items) {
  EnsembleArgs b = b0;
  if constexpr (SWEEP) {
    if (!ens_sweep_args(b, (unsigned)__builtin_amdgcn_readfirstlane(b0.item_world[blockIdx.x]))) return;
  }
  const uint4 item = items[blockIdx.x];
  const size_t body_row0 = (size_t)(unsigned)__builtin_amdgcn_readfirstlane(item.x);
  const int n = (int)__builtin_amdgcn_readfirstlane(item.y);
  const size_t tracer_row0 = (size_t)(unsigned)__builtin_amdgcn_readfirstlane(item.z);
  const int count = (int)__builtin_amdgcn_readfirstlane(item.w);
  TracerRows rows;
  rows.tpos = t.tpos, rows.tvel = t.tvel, rows.tacc_out = t.tacc_out;
  rst_world_tile<R>(b, rows, n, body_row0, tracer_row0, count);
}

}  // namespace

hipError_t launch_rr_tracers(hipStream_t s, int64_t blocks, size_t lds_bytes, const uint4* items, const EnsembleArgs& bodies,
                             const RrTracerArgs& t) {
  if (blocks < 1 || blocks > kEnsembleMaxRows || !items || lds_bytes > ensemble_lds_bytes(kEnsembleMaxBodies) || !t.tpos ||
      !bodies.pos_in || !bodies.mass)
    return hipErrorInvalidValue;
  if (bodies.sweep) {
    if (!bodies.item_world || !t.tvel) return hipErrorInvalidValue;  // (a sweep is a step)
    hipLaunchKernelGGL((rr_tracers<kRestrictedPerLane, true>), dim3((unsigned)blocks), dim3(kEnsembleBlock), lds_bytes, s, bodies, t, items);
  } else {
    hipLaunchKernelGGL((rr_tracers<kRestrictedPerLane, false>), dim3((unsigned)blocks), dim3(kEnsembleBlock), lds_bytes, s, bodies, t, items);
  }
  return hipGetLastError();
}

}  // namespace nbody
