// Resident runs in f64 (nbody_resident_ensemble64, nbody_resident_ragged64): one block per world, the world in LDS for up to
// kResidentStepsPerLaunch steps of a sweep (ensemble_resident.h), as ensemble_resident.hip does it in f32.
//
// A step is the stepping kernel's step (ensemble64_kernels.hip) from the same text: ens64_exact_sum, or ens64_fast_sum (which
// ends in ens_group_sum), of ensemble64_world.h over the same LDS layout — rows padded to 8 with NaN positions, which nothing
// here writes — under the route ens64_sweep_args takes from the world's entry, and ens_integrate's expression.  Positions are
// stored over the old ones in LDS after every step; velocities live in LDS behind the weights, because a target's owner is lane
// t in the EXACT arm and lane t * SPLIT in the FAST arm and a world changes arm between steps when it leaves or enters FAST's
// domain.  Two barriers per step, which every thread reaches (the EXACT arm is a branch here, not an early return).
//
// No static LDS, as in every f64 ensemble kernel: FAST's decision for step s + 1 — the OR of outside_fast over the positions
// that step s stores — goes through a borrowed word and the step's own second barrier.  The borrowed words are the two halves
// of the LDS slot of target 0's velocity.x: target 0's owner is thread 0 in both arms, so thread 0 keeps that velocity in
// registers for the whole launch and the slot is free.  Step s uses word s & 1: the owners' waves that store a position outside
// the domain write 1 into it between the step's barriers, thread 0 clears the other word at the same time, every thread reads
// the word after the second barrier.  Nobody reads word s & 1 before that barrier, and its next writer (the clear of step
// s + 1) comes after the first barrier of step s + 1, which every reader has passed.  Step 0's decision comes from the staging
// (ens64_stage_world, which borrows a weight for it as the stepping kernel does).
//
// This translation unit is compiled with -ffp-contract=off: nothing fuses unless written as an fma.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nbody_hip.h"
#include "ensemble64_kernels.h"
#include "ensemble64_world.h"
#include "ensemble_resident.h"

namespace nbody {
namespace {

template <int SPLIT>
__device__ __forceinline__ void ens64_resident_block(const Ensemble64Args& launch, const int n, const size_t row0, const unsigned world) {
  constexpr int TPB = kEnsembleBlock / SPLIT;  // targets per block: >= n
  Ensemble64Args a = launch;
  if (!ens64_sweep_args(a, world)) return;  // (a.step >= steps: before any barrier)
  const int left = a.sweep[__builtin_amdgcn_readfirstlane(world)].steps - a.step;
  const int count = left < kResidentStepsPerLaunch ? left : kResidentStepsPerLaunch;

  extern __shared__ __attribute__((aligned(16))) unsigned char ens64_resident_lds[];
  const Ens64WorldLds w(ens64_resident_lds, n);
  double2* const svel = reinterpret_cast<double2*>(w.sw + w.npad);  // (behind the weights: ensemble64_lds_bytes(n) into the block's LDS, a multiple of 160)
  uint32_t* const flag = reinterpret_cast<uint32_t*>(svel);  // flag[0], flag[1]: the slot of target 0's velocity.x
  double2* const gpos = const_cast<double2*>(a.pos_in);       // (the handle's current buffer: read by the staging, written at the end)
  const int fast = a.fast;
  const int tid = (int)threadIdx.x;

  double2 v0 = double2{0.0, 0.0};  // thread 0: target 0's velocity
  for (int s = tid; s < n; s += kEnsembleBlock) {
    const double2 v = a.vel[row0 + s];
    if (s == 0) {
      v0 = v;
      flag[0] = flag[1] = 0u;
    } else {
      svel[s] = v;
    }
  }
  int hazard = ens64_stage_world(w, a.pos_in, a.weight, row0, fast);  // (its first barrier covers the velocities too)
  const double clamp = a.clamp, delta = a.delta;

  for (int step = 0; step < count; ++step) {
    double tx = 0.0, ty = 0.0, sx = 0.0, sy = 0.0;  // the target's position and its acceleration, in its owner
    bool own = false;
    int t = 0;
    if (hazard) {
      // ---- EXACT: thread = target
      t = tid;
      own = tid < TPB && t < n;
      if (own) {
        const double2 p = w.spos[t];
        tx = p.x, ty = p.y;
        ens64_exact_sum(w, p.x, p.y, clamp, sx, sy);
      }
    } else {
      // ---- FAST: SPLIT consecutive lanes per target
      const int part = tid % SPLIT;
      t = tid / SPLIT;
      const bool live = t < n;
      const double2 p = w.spos[live ? t : 0];
      double px[1] = {p.x}, py[1] = {p.y}, ax[1], ay[1];
      ens64_fast_sum<SPLIT, 1>(w, part, px, py, clamp, ax, ay);
      tx = p.x, ty = p.y, sx = ax[0], sy = ay[0];
      own = live && part == 0;
    }
    double2 v = double2{0.0, 0.0}, x = double2{0.0, 0.0};
    int bad = 0;
    if (own) {
      v = svel[t];
      if (t == 0) v = v0;  // (the slot holds the flags)
      ens_resident_integrate(delta, tx, ty, sx, sy, v, x);
      bad = (int)outside_fast(x.x) | (int)outside_fast(x.y);
    }
    __syncthreads();  // every lane has read this step's sources
    if (own) {
      w.spos[t] = x;
      if (t == 0) v0 = v; else svel[t] = v;
    }
    if (fast) {  // (uniform)
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
    gpos[row0 + s] = w.spos[s];
    double2 v = svel[s];
    if (s == 0) v = v0;
    a.vel[row0 + s] = v;
  }
}

template <int SPLIT>
__global__ __launch_bounds__(kEnsembleBlock) void ensemble64_resident(const Ensemble64Args a) {
  const int n = a.n_bodies;
  ens64_resident_block<SPLIT>(a, n, (size_t)blockIdx.x * (size_t)n, blockIdx.x);
}

// Ragged: the world's {row0, n} is the same in every lane, so the switch on its lane split is taken by the whole block.
__global__ __launch_bounds__(kEnsembleBlock) void ensemble64_resident_ragged(const Ensemble64Args a, const uint2* __restrict__ worlds) {
  const uint2 item = worlds[blockIdx.x];
  const size_t row0 = (size_t)(unsigned)__builtin_amdgcn_readfirstlane(item.x);
  const int n = (int)__builtin_amdgcn_readfirstlane(item.y);
  switch (ensemble_split(n)) {
    case 1: ens64_resident_block<1>(a, n, row0, blockIdx.x); break;
    case 2: ens64_resident_block<2>(a, n, row0, blockIdx.x); break;
    case 4: ens64_resident_block<4>(a, n, row0, blockIdx.x); break;
    case 8: ens64_resident_block<8>(a, n, row0, blockIdx.x); break;
    case 16: ens64_resident_block<16>(a, n, row0, blockIdx.x); break;
    case 32: ens64_resident_block<32>(a, n, row0, blockIdx.x); break;
    default: ens64_resident_block<64>(a, n, row0, blockIdx.x); break;
  }
}

}  // namespace

hipError_t launch_ensemble64_resident(hipStream_t s, int64_t n_worlds, const uint2* worlds, size_t lds_bytes, Ensemble64Args a) {
  if (n_worlds < 1 || n_worlds > kEnsembleMaxRows || !a.sweep || !a.pos_in || !a.vel || lds_bytes > ensemble64_resident_lds_bytes(kResidentMaxBodies))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)n_worlds), block(kEnsembleBlock);
  if (worlds) {
    hipLaunchKernelGGL(ensemble64_resident_ragged, grid, block, lds_bytes, s, a, worlds);
    return hipGetLastError();
  }
  if (a.n_bodies < 1 || a.n_bodies > kResidentMaxBodies || lds_bytes < ensemble64_resident_lds_bytes(a.n_bodies)) return hipErrorInvalidValue;
  switch (ensemble_split(a.n_bodies)) {
    case 1: hipLaunchKernelGGL(ensemble64_resident<1>, grid, block, lds_bytes, s, a); break;
    case 2: hipLaunchKernelGGL(ensemble64_resident<2>, grid, block, lds_bytes, s, a); break;
    case 4: hipLaunchKernelGGL(ensemble64_resident<4>, grid, block, lds_bytes, s, a); break;
    case 8: hipLaunchKernelGGL(ensemble64_resident<8>, grid, block, lds_bytes, s, a); break;
    case 16: hipLaunchKernelGGL(ensemble64_resident<16>, grid, block, lds_bytes, s, a); break;
    case 32: hipLaunchKernelGGL(ensemble64_resident<32>, grid, block, lds_bytes, s, a); break;
    default: hipLaunchKernelGGL(ensemble64_resident<64>, grid, block, lds_bytes, s, a); break;
  }
  return hipGetLastError();
}

}  // namespace nbody
