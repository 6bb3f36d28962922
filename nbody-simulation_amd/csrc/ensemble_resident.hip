// Resident runs in f32 (nbody_resident_ensemble, nbody_resident_ragged): one block per world, the world in LDS for up to
// kResidentStepsPerLaunch steps of a sweep (ensemble_resident.h).
//
// What a step computes is the stepping kernel's step (ensemble_kernels.hip), from the same text: ens_exact_sum, or ens_fast_sum
// and ens_group_sum, of ensemble_world.h / ensemble_device.h over the same LDS layout, under the route ens_sweep_args takes from
// the world's entry, and ens_integrate's expression.  What differs is where a step's operands come from and its results go:
//   positions, masses   staged once by ens_stage_world; a step's new positions are stored over the old ones in LDS;
//   velocities          in LDS behind the masses, not in the owner's registers: a target's owner is lane t in the EXACT arm and
//                       lane t * SPLIT in the FAST arm, and under AUTO a world changes arm from one step to the next;
//   AUTO's decision     of step s + 1 is the OR of outside_fast over the positions that step s stores, which is the OR over the
//                       positions at the start of step s + 1: the owners take it on the values they store and the step's second
//                       barrier carries it, so AUTO costs no barrier of its own (__syncthreads_or is three).  It goes through
//                       two words of static LDS, word s & 1 in step s: between the step's barriers the waves that store a
//                       position outside the domain write 1 into it and thread 0 clears the other word; every thread reads it
//                       after the second barrier.  Nobody reads word s & 1 before that barrier, and its next writer (the clear
//                       of step s + 1) comes after the first barrier of step s + 1, which every reader has passed.  Step 0's
//                       decision comes from the staging, as in the stepping kernel;
//   barriers            two per step: every lane has read the step's sources | the owners store | every lane sees the stores.
//                       Every thread reaches both: the EXACT arm here is a branch, not the early return of ens_world_tile.
// A world that has no step left in this launch returns before any barrier and touches nothing: its bits stay.  After its last
// step of the launch the block writes positions and velocities over its own rows, which no other block reads or writes.
//
// This translation unit is compiled with -ffp-contract=off: nothing fuses unless written as an fma.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nbody_hip.h"
#include "ensemble_device.h"
#include "ensemble_kernels.h"
#include "ensemble_resident.h"
#include "ensemble_world.h"

namespace nbody {
namespace {

// The steps of world `world` (rows row0 .. row0 + n, n <= kResidentMaxBodies, so one tile) that this launch takes.  Every
// thread of the block calls it (it holds barriers).
template <int SPLIT>
__device__ __forceinline__ void ens_resident_block(const EnsembleArgs& launch, const int n, const size_t row0, const unsigned world) {
  constexpr int TPB = kEnsembleBlock / SPLIT;  // targets per block: >= n
  EnsembleArgs a = launch;
  if (!ens_sweep_args(a, world)) return;  // (a.step >= steps: before any barrier)
  const int left = a.sweep[__builtin_amdgcn_readfirstlane(world)].steps - a.step;
  const int count = left < kResidentStepsPerLaunch ? left : kResidentStepsPerLaunch;

  extern __shared__ __attribute__((aligned(16))) unsigned char ens_resident_lds[];
  const EnsWorldLds w(ens_resident_lds, n);
  float2* const svel = reinterpret_cast<float2*>(w.massf + 2 * w.nc);  // (behind the masses: ensemble_lds_bytes(n) into the block's LDS)
  float2* const gpos = const_cast<float2*>(a.pos_in);  // (the handle's current buffer: read by the staging, written at the end)
  const bool decide = a.arith == NBODY_ARITH_AUTO;
  const int tid = (int)threadIdx.x;

  __shared__ uint32_t flag[2];  // AUTO's decision of the next step (above)
  if (tid == 0) flag[0] = flag[1] = 0u;
  for (int s = tid; s < n; s += kEnsembleBlock) svel[s] = a.vel[row0 + s];
  int hazard = ens_stage_world(w, a.pos_in, a.mass, row0, decide);  // (its barrier covers the velocities and the flags too)
  const float clamp = a.clamp, delta = a.delta;

  for (int step = 0; step < count; ++step) {
    float px[1], py[1], ax[1], ay[1];
    bool own = false;
    int t = 0;
    if (a.arith == NBODY_ARITH_EXACT || hazard) {
      // ---- EXACT: thread = target, j ascending
      t = tid;
      own = tid < TPB && t < n;
      if (own) {
        const float2 p = w.body(t);
        px[0] = p.x, py[0] = p.y;
        ens_exact_sum<1>(w, px, py, clamp, ax, ay);
      }
    } else {
      // ---- FAST: SPLIT consecutive lanes per target
      const int part = tid % SPLIT;
      t = tid / SPLIT;
      const bool live = t < n;
      const float2 p = w.body(live ? t : 0);
      px[0] = p.x, py[0] = p.y;
      ens_fast_sum<SPLIT, 1>(w, part, px, py, clamp, ax, ay);
      ax[0] = ens_group_sum<SPLIT>(ax[0]);
      ay[0] = ens_group_sum<SPLIT>(ay[0]);
      own = live && part == 0;
    }
    float2 v = make_float2(0.f, 0.f), x = make_float2(0.f, 0.f);
    int bad = 0;
    if (own) {
      v = svel[t];
      ens_resident_integrate(delta, px[0], py[0], ax[0], ay[0], v, x);
      bad = (int)outside_fast(x.x) | (int)outside_fast(x.y);
    }
    __syncthreads();  // every lane has read this step's sources
    if (own) {
      const int o = 4 * (t >> 1) + (t & 1);
      w.cplf[o] = x.x;
      w.cplf[o + 2] = x.y;
      svel[t] = v;
    }
    if (decide) {  // (uniform)
      const int word = step & 1;
      if (tid == 0) flag[word ^ 1] = 0u;
      if (__builtin_amdgcn_ballot_w64(bad != 0) != 0 && (tid & 63) == 0) flag[word] = 1u;
      __syncthreads();  // every lane sees the stores
      hazard = __builtin_amdgcn_readfirstlane((int)flag[word]);  // (the same in every lane: says so to the compiler)
    } else {
      __syncthreads();
    }
  }

  for (int s = tid; s < n; s += kEnsembleBlock) {
    gpos[row0 + s] = w.body(s);
    a.vel[row0 + s] = svel[s];
  }
}

template <int SPLIT>
__global__ __launch_bounds__(kEnsembleBlock) void ensemble_resident(const EnsembleArgs a) {
  const int n = a.n_bodies;
  ens_resident_block<SPLIT>(a, n, (size_t)blockIdx.x * (size_t)n, blockIdx.x);
}

// Ragged: the world's {row0, n} is the same in every lane (a scalar load), so the switch on its lane split is taken by the
// whole block, as in ensemble_step_ragged.
__global__ __launch_bounds__(kEnsembleBlock) void ensemble_resident_ragged(const EnsembleArgs a, const uint2* __restrict__ worlds) {
  const uint2 item = worlds[blockIdx.x];
  const size_t row0 = (size_t)(unsigned)__builtin_amdgcn_readfirstlane(item.x);
  const int n = (int)__builtin_amdgcn_readfirstlane(item.y);
  switch (ensemble_split(n)) {
    case 1: ens_resident_block<1>(a, n, row0, blockIdx.x); break;
    case 2: ens_resident_block<2>(a, n, row0, blockIdx.x); break;
    case 4: ens_resident_block<4>(a, n, row0, blockIdx.x); break;
    case 8: ens_resident_block<8>(a, n, row0, blockIdx.x); break;
    case 16: ens_resident_block<16>(a, n, row0, blockIdx.x); break;
    case 32: ens_resident_block<32>(a, n, row0, blockIdx.x); break;
    default: ens_resident_block<64>(a, n, row0, blockIdx.x); break;
  }
}

}  // namespace

hipError_t launch_ensemble_resident(hipStream_t s, int64_t n_worlds, const uint2* worlds, size_t lds_bytes, EnsembleArgs a) {
  if (n_worlds < 1 || n_worlds > kEnsembleMaxRows || !a.sweep || !a.pos_in || !a.vel || lds_bytes > ensemble_resident_lds_bytes(kResidentMaxBodies))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)n_worlds), block(kEnsembleBlock);
  if (worlds) {
    hipLaunchKernelGGL(ensemble_resident_ragged, grid, block, lds_bytes, s, a, worlds);
    return hipGetLastError();
  }
  if (a.n_bodies < 1 || a.n_bodies > kResidentMaxBodies || lds_bytes < ensemble_resident_lds_bytes(a.n_bodies)) return hipErrorInvalidValue;
  switch (ensemble_split(a.n_bodies)) {
    case 1: hipLaunchKernelGGL(ensemble_resident<1>, grid, block, lds_bytes, s, a); break;
    case 2: hipLaunchKernelGGL(ensemble_resident<2>, grid, block, lds_bytes, s, a); break;
    case 4: hipLaunchKernelGGL(ensemble_resident<4>, grid, block, lds_bytes, s, a); break;
    case 8: hipLaunchKernelGGL(ensemble_resident<8>, grid, block, lds_bytes, s, a); break;
    case 16: hipLaunchKernelGGL(ensemble_resident<16>, grid, block, lds_bytes, s, a); break;
    case 32: hipLaunchKernelGGL(ensemble_resident<32>, grid, block, lds_bytes, s, a); break;
    default: hipLaunchKernelGGL(ensemble_resident<64>, grid, block, lds_bytes, s, a); break;
  }
  return hipGetLastError();
}

}  // namespace nbody
