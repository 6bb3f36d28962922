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
template <int R>
__global__ __launch_bounds__(kEnsembleBlock) void rr_tracers(const EnsembleArgs b, const RrTracerArgs t, const uint4* __restrict__ items) {
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
  hipLaunchKernelGGL(rr_tracers<kRestrictedPerLane>, dim3((unsigned)blocks), dim3(kEnsembleBlock), lds_bytes, s, bodies, t, items);
  return hipGetLastError();
}

}  // namespace nbody
