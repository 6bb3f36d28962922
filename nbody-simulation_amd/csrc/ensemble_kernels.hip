// Ensemble step: worlds x target tiles in one launch, a world's sources staged whole in LDS (ensemble_kernels.h).
//
// What every world computes is the direct step (direct_kernels.hip):
//   a_i = sum_j calculate_gravity(p_i, p_j, w_j) over the bodies of its own world      src/main.rs:234-253
//   v_i += a_i*dt ; x_i += v_i*dt                                                        src/main.rs:419-423
// EXACT  one thread per target, one ascending-j chain of pair_as_written<float> (pair.h: IEEE divide through div_pair, the
//        is_normal skip, no contraction): bit-identical to the oracle's update_direct of that world alone.
// FAST   direct_kernels.hip's pair (one v_rcp_f32, fused multiply-adds, the 2^-90 biased denominator) over source COUPLES
//        {xA, xB, yA, yB}: every multiply-add is a packed op over two sources (a packed op fills its 4-cycle
//        issue slot with two values per lane); per couple 2 v_pk_add, 2 v_pk_mul, 4 v_pk_fma, 2 v_add, 2 v_max, 2 v_rcp.
//        Order of additions, a function of n_bodies alone: with SPLIT = ensemble_split(n) lanes per target, lane `part` takes
//        the couples part, part + SPLIT, ... in ascending order; the even and the odd sources of its couples are summed apart,
//        64 couples at a time (two-level summation: each run of 64 couples is added as one value to the lane's running
//        total, even half first); the SPLIT totals meet in a butterfly — lanes ^1, ^2, mirrored within 8, ^8, rows of 16, halves
//        of the wave — whose additions are commutative pairs, so every lane of the group ends with the same bits.
//        Worst case 64 + 32 + 6 roundings of 2^-24 on sum |term| at n = 4096 (6e-6), against the 2e-5 of tests/_tol.py.
// AUTO   every block of a world stages all of that world's rows, so it sees every position of the world: the block-wide OR of
//        outside_fast() over the rows it loads IS the world's decision for this step, the same in each of the world's blocks.
//        No flag buffer, no extra kernel, nothing read back.
// Padding: an odd n leaves the last couple's second source at (0, 0) with mass 0: FAST adds exactly 0 for it (s = 0 * rcp),
// EXACT never reads it.  Lanes past the end of a world compute target 0 again (the butterfly needs every lane) and store nothing.
//
// This translation unit is compiled with -ffp-contract=off: nothing fuses unless written as an fma.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nbody_hip.h"
#include "ensemble_device.h"
#include "ensemble_kernels.h"
#include "ensemble_world.h"

namespace nbody {
namespace {

// What a block computes: one tile of the targets of the world whose rows are row0 .. row0 + n — its sources staged in LDS with
// the AUTO decision taken on the way, then the EXACT or the FAST arm (ensemble_world.h has the staging and both sums).  A
// function of the world through (n, row0, tile) alone: the uniform kernel and the ragged one share it, and with it every bit.
// Every thread of the block calls it (it holds a barrier).
template <int SPLIT>
__device__ __forceinline__ void ens_world_tile(const EnsembleArgs& a, const int n, const size_t row0, const unsigned tile) {
  constexpr int TPB = kEnsembleBlock / SPLIT;  // targets per block
  extern __shared__ __attribute__((aligned(16))) unsigned char ens_lds[];
  const EnsWorldLds w(ens_lds, n);

  // ---- the world's sources into LDS, and its AUTO decision on the way
  const int hazard = ens_stage_world(w, a.pos_in, a.mass, row0, a.arith == NBODY_ARITH_AUTO);
  const float clamp = a.clamp;
  float px[1], py[1], ax[1], ay[1];

  if (a.arith == NBODY_ARITH_EXACT || hazard) {
    // ---- EXACT: thread = target, j ascending (no barrier follows: threads without a target leave)
    if ((int)threadIdx.x >= TPB) return;
    const int t = (int)tile * TPB + (int)threadIdx.x;
    if (t >= n) return;
    const float2 p = w.body(t);
    px[0] = p.x, py[0] = p.y;
    ens_exact_sum<1>(w, px, py, clamp, ax, ay);
    ens_integrate(a, row0 + t, px[0], py[0], ax[0], ay[0]);
    return;
  }

  // ---- FAST: SPLIT consecutive lanes per target
  const int part = (int)threadIdx.x % SPLIT;
  const int t = (int)tile * TPB + (int)threadIdx.x / SPLIT;
  const bool live = t < n;
  const float2 p = w.body(live ? t : 0);
  px[0] = p.x, py[0] = p.y;
  ens_fast_sum<SPLIT, 1>(w, part, px, py, clamp, ax, ay);
  const float sx = ens_group_sum<SPLIT>(ax[0]);
  const float sy = ens_group_sum<SPLIT>(ay[0]);
  if (live && part == 0) ens_integrate(a, row0 + t, px[0], py[0], sx, sy);
}

// Sweeps (nbody_sweep_*): the same block body under the world's own parameters.  The world's entry is read once per block; its
// index is the same in every lane, so the entry arrives by scalar loads and everything decided from it is decided block-wide:
//   finished (a.step >= steps)  the positions are double-buffered and the handle flips the buffers once per launch for all
//                               worlds, so the block carries its own tile of pos_in over to pos_out as raw bits and returns
//                               before anything is staged and before any barrier.  Velocities are not touched.
//   route                       the clamp test of direct_arith_f32, taken here on the world's clamp: a world whose clamp is
//                               below kFastClampFloor (or NaN) is EXACT for the call, in every one of its blocks (and in its
//                               tracers' blocks, which take the same test on the same entry); its neighbours are not asked.
//   delta, clamp                replace the launch's in a copy of the arguments: ens_world_tile runs as it is.
// (ens_sweep_args of ensemble_world.h is the entry's reading, shared with the tracers' kernels.)
// The plain launches are the SWEEP = false instantiations: they read nothing of this and compile to what they were.
template <int SPLIT>
__device__ __forceinline__ void ens_carry_tile(const EnsembleArgs& a, const int n, const size_t row0, const unsigned tile) {
  constexpr int TPB = kEnsembleBlock / SPLIT;
  const int t = (int)tile * TPB + (int)threadIdx.x;
  if ((int)threadIdx.x >= TPB || t >= n) return;
  const unsigned long long* in = reinterpret_cast<const unsigned long long*>(a.pos_in);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(a.pos_out);
  out[row0 + t] = in[row0 + t];
}

template <int SPLIT, bool SWEEP>
__device__ __forceinline__ void ens_step_block(const EnsembleArgs& a, const int n, const size_t row0, const unsigned tile, const unsigned world) {
  if constexpr (SWEEP) {
    EnsembleArgs b = a;
    if (!ens_sweep_args(b, world)) {
      ens_carry_tile<SPLIT>(a, n, row0, tile);
      return;
    }
    ens_world_tile<SPLIT>(b, n, row0, tile);
  } else {
    ens_world_tile<SPLIT>(a, n, row0, tile);
  }
}

template <int SPLIT, bool SWEEP>
__global__ __launch_bounds__(kEnsembleBlock) void ensemble_step(const EnsembleArgs a) {
  const int n = a.n_bodies;
  const unsigned world = blockIdx.x / a.tiles, tile = blockIdx.x - world * a.tiles;
  ens_step_block<SPLIT, SWEEP>(a, n, (size_t)world * (size_t)n, tile, world);
}

// Ragged: the block's work item {row0, n | tile << 16} is the same in every lane (a scalar load), so the switch on the
// world's lane split is taken by the whole block — the barrier of the staging and the butterfly of FAST see every thread.
// Under a sweep the item's world comes from a.item_world, a table beside the items' (their layout has no room for it), by the
// same kind of load.
template <bool SWEEP>
__global__ __launch_bounds__(kEnsembleBlock) void ensemble_step_ragged(const EnsembleArgs a, const uint2* __restrict__ items) {
  const uint2 item = items[blockIdx.x];
  const size_t row0 = (size_t)(unsigned)__builtin_amdgcn_readfirstlane(item.x);
  const unsigned packed = __builtin_amdgcn_readfirstlane(item.y);
  const int n = (int)(packed & 0xffffu);
  const unsigned tile = packed >> 16;
  unsigned world = 0;
  if constexpr (SWEEP) world = __builtin_amdgcn_readfirstlane(a.item_world[blockIdx.x]);
  switch (ensemble_split(n)) {
    case 1: ens_step_block<1, SWEEP>(a, n, row0, tile, world); break;
    case 2: ens_step_block<2, SWEEP>(a, n, row0, tile, world); break;
    case 4: ens_step_block<4, SWEEP>(a, n, row0, tile, world); break;
    case 8: ens_step_block<8, SWEEP>(a, n, row0, tile, world); break;
    case 16: ens_step_block<16, SWEEP>(a, n, row0, tile, world); break;
    case 32: ens_step_block<32, SWEEP>(a, n, row0, tile, world); break;
    default: ens_step_block<64, SWEEP>(a, n, row0, tile, world); break;
  }
}

}  // namespace

hipError_t launch_ensemble_step(hipStream_t s, int64_t n_worlds, EnsembleArgs a) {
  if (n_worlds < 1 || a.n_bodies < 1 || a.n_bodies > kEnsembleMaxBodies || n_worlds * a.n_bodies > kEnsembleMaxRows) return hipErrorInvalidValue;
  if (a.sweep && (!a.pos_out || !a.vel)) return hipErrorInvalidValue;  // (a sweep is a step: a finished world writes pos_out)
  const int split = ensemble_split(a.n_bodies);
  const int tpb = kEnsembleBlock / split;
  a.tiles = (unsigned)((a.n_bodies + tpb - 1) / tpb);
  const dim3 grid((unsigned)(n_worlds * a.tiles));  // <= 2^26 blocks
  const size_t lds = ensemble_lds_bytes(a.n_bodies);
#define NB_ENS_GO(S)                                                                    \
  do {                                                                                  \
    if (a.sweep) {                                                                      \
      hipLaunchKernelGGL((ensemble_step<S, true>), grid, dim3(kEnsembleBlock), lds, s, a);  \
    } else {                                                                            \
      hipLaunchKernelGGL((ensemble_step<S, false>), grid, dim3(kEnsembleBlock), lds, s, a); \
    }                                                                                   \
  } while (0)
  switch (split) {
    case 1: NB_ENS_GO(1); break;
    case 2: NB_ENS_GO(2); break;
    case 4: NB_ENS_GO(4); break;
    case 8: NB_ENS_GO(8); break;
    case 16: NB_ENS_GO(16); break;
    case 32: NB_ENS_GO(32); break;
    default: NB_ENS_GO(64); break;
  }
#undef NB_ENS_GO
  return hipGetLastError();
}

hipError_t launch_ensemble_step_ragged(hipStream_t s, int64_t blocks, size_t lds_bytes, const uint2* items, EnsembleArgs a) {
  if (blocks < 1 || blocks > kEnsembleMaxRows || !items || lds_bytes > ensemble_lds_bytes(kEnsembleMaxBodies)) return hipErrorInvalidValue;
  if (a.sweep && (!a.item_world || !a.pos_out || !a.vel)) return hipErrorInvalidValue;
  if (a.sweep) {
    hipLaunchKernelGGL(ensemble_step_ragged<true>, dim3((unsigned)blocks), dim3(kEnsembleBlock), lds_bytes, s, a, items);
  } else {
    hipLaunchKernelGGL(ensemble_step_ragged<false>, dim3((unsigned)blocks), dim3(kEnsembleBlock), lds_bytes, s, a, items);
  }
  return hipGetLastError();
}

}  // namespace nbody
