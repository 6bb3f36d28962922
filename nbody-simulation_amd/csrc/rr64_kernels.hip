// Ragged restricted ensembles in f64: the tracers' step from a table of work items (rr64_kernels.h).
//
// What every tracer computes is what restricted64_kernels.hip states, in double:
//   a_t = sum_j calculate_gravity(p_t, p_j, w_j as f64) over the bodies of its own world, j ascending      src/main.rs:234-253
//   v_t += a_t*dt ; x_t += v_t*dt                                                                          src/main.rs:419-423
// and the block's body is the same text, rst64_world_tile (restricted64_device.h): this kernel only reads which world and which
// of its tracers a block is from its work item, where the uniform kernel computes them from blockIdx.
//
// This translation unit is compiled with -ffp-contract=off: nothing fuses unless written as an fma.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nbody_hip.h"
#include "restricted64_device.h"
#include "rr64_kernels.h"

namespace nbody {
namespace {

// The block's work item {body_row0, n, tracer_row0, count} is the same in every lane (a scalar load), so n and count are
// uniform: the barriers of the staging see every thread.  Dynamic LDS is the launch's; the kernel uses no other.
// SWEEP (nbody_sweep_*): the item's world from b0.item_world, a table beside the items' (by the same kind of load), and with it
// the world's own delta, clamp and route (ens64_sweep_args); the blocks of a world that has taken its steps return at once.
template <int R, bool SWEEP>
__global__ __launch_bounds__(kEnsembleBlock) void rr64_tracers(const Ensemble64Args b0, const Rr64TracerArgs t, const uint4* __restrict__ items) {
  Ensemble64Args b = b0;
  if constexpr (SWEEP) {
    if (!ens64_sweep_args(b, (unsigned)__builtin_amdgcn_readfirstlane(b0.item_world[blockIdx.x]))) return;
  }
  const uint4 item = items[blockIdx.x];
  const size_t body_row0 = (size_t)(unsigned)__builtin_amdgcn_readfirstlane(item.x);
  const int n = (int)__builtin_amdgcn_readfirstlane(item.y);
  const size_t tracer_row0 = (size_t)(unsigned)__builtin_amdgcn_readfirstlane(item.z);
  const int count = (int)__builtin_amdgcn_readfirstlane(item.w);
  Tracer64Rows rows;
  rows.tpos = t.tpos, rows.tvel = t.tvel, rows.tacc_out = t.tacc_out;
  rst64_world_tile<R>(b, rows, n, body_row0, tracer_row0, count);
}

}  // namespace

hipError_t launch_rr64_tracers(hipStream_t s, int64_t blocks, size_t lds_bytes, const uint4* items, const Ensemble64Args& bodies,
                               const Rr64TracerArgs& t) {
  if (blocks < 1 || blocks > kEnsembleMaxRows || !items || lds_bytes > ensemble64_lds_bytes(kEnsembleMaxBodies) || !t.tpos ||
      !bodies.pos_in || !bodies.weight)
    return hipErrorInvalidValue;
  if (lds_bytes > 65536) {  // its own function, so its own limit: the uniform kernel's and the bodies' raised ones do not cover it
    static std::atomic<bool> raised[64], raised_sweep[64];
    const hipError_t h = bodies.sweep ? ens64_raise_lds_limit(reinterpret_cast<const void*>(&rr64_tracers<kRestricted64PerLane, true>), raised_sweep)
                                      : ens64_raise_lds_limit(reinterpret_cast<const void*>(&rr64_tracers<kRestricted64PerLane, false>), raised);
    if (h != hipSuccess) return h;
  }
  if (bodies.sweep) {
    if (!bodies.item_world || !t.tvel) return hipErrorInvalidValue;  // (a sweep is a step)
    hipLaunchKernelGGL((rr64_tracers<kRestricted64PerLane, true>), dim3((unsigned)blocks), dim3(kEnsembleBlock), lds_bytes, s, bodies, t, items);
  } else {
    hipLaunchKernelGGL((rr64_tracers<kRestricted64PerLane, false>), dim3((unsigned)blocks), dim3(kEnsembleBlock), lds_bytes, s, bodies, t, items);
  }
  return hipGetLastError();
}

}  // namespace nbody
