// Ensemble step in f64: worlds x target tiles in one launch, a world's sources staged whole in LDS (ensemble64_kernels.h).
//
// What every world computes is the f64 direct step (direct64.hip):
//   a_i = sum_j calculate_gravity(p_i, p_j, w_j as f64) over the bodies of its own world, in double      src/main.rs:234-253
//   v_i += a_i*dt ; x_i += v_i*dt                                                                        src/main.rs:419-423
// EXACT  one thread per target.  The terms of kEns64TermBlock sources are evaluated first, branch-free (pair_term_select,
//        pair.h: two IEEE divisions, the is_normal skip as a select), and then added in ascending j — one chain of IEEE
//        additions per target, bit-identical to the oracle's update_direct of that world alone; the block's division chains
//        are independent and overlap (the kernel is bound by the two compiler-expanded f64 divisions per pair).  The pad that
//        completes the last term block has NaN positions: its pairs are skipped, a -0.0 term, the identity of IEEE addition.
// FAST   pair_fast(double...) of pair.h: v_rcp_f64 plus one Newton step, fused multiply-adds, the 2^-700 biased denominator.
//        Order of additions, a function of n_bodies alone: with SPLIT = ensemble_split(n) lanes per target, lane `part` takes
//        the sources part, part + SPLIT, part + 2 SPLIT, ... in ascending order, kEns64Run = 64 of them at a time (a run).
//        Within a run the lane's 1st, 3rd, ... source accumulate by fma into one sum and its 2nd, 4th, ... into another (two
//        independent chains); the run ends with total = total + (sum_odd_places + sum_even_places) — two-level summation.
//        The SPLIT totals then meet in a butterfly — lanes ^1, ^2, mirrored within 8, ^8, rows of 16, halves of the wave —
//        each step the sum of a value and its partner's (the same two operands in both lanes), so every lane of the group
//        ends with the same bits.  A 64-bit value crosses lanes as two 32-bit DPP / permlane moves.
//        Rounding count, worst case n = 4096 (SPLIT 1, 64 runs): 32 fma roundings inside a run's chain, 1 to join its two
//        chains, 64 to add the runs: 97 roundings of 2^-53 on sum |term|, 1.08e-14.  (Smaller n: at most 32 + 1 + ceil(n /
//        (64 SPLIT)) + log2 SPLIT, never more.)  A FAST term differs from the reference's by at most 16 roundings (fma'd
//        d2 and denominator, reciprocal + Newton <= 2 ulp, force * r, against the reference's two products, sum, product and
//        division; the bias is below 2^-199 of any denominator, direct64.h).  (97 + 16) * 2^-53 = 1.25e-14 of sum |term|
//        from the exact sum of the reference's terms; the oracle's own double chain that the tests compare with is within
//        4095 * 2^-53 = 4.55e-13 of that sum in the worst case, so 4.7e-13 against it — a bound, under the contract's 1e-12.
//        Lanes past the end of a world compute target 0 again (the butterfly needs every lane) and store nothing; FAST reads
//        no padding.
// Route  FAST is opt-in (args.fast).  Every block of a world stages all of that world's rows, so it sees every position of the
//        world: the block-wide OR of outside_fast() over the rows it loads IS the world's decision for this step, the same in
//        each of the world's blocks.  No flag buffer, no extra kernel, nothing read back.  The OR goes through one borrowed
//        word of the staged weights and plain barriers, not __syncthreads_or: the kernel has no static LDS at all.
//
// The staging, the EXACT chain and the FAST sum are written once in ensemble64_world.h, which the tracers' kernel of the
// restricted ensemble (restricted64_kernels.hip) runs too.
//
// This translation unit is compiled with -ffp-contract=off: nothing fuses unless written as an fma.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nbody_hip.h"
#include "ensemble64_kernels.h"
#include "ensemble64_world.h"

namespace nbody {
namespace {

// What a block computes: one tile of the targets of the world whose rows are row0 .. row0 + n — its sources staged in LDS with
// FAST's decision taken on the way, then the EXACT or the FAST arm, all three from ensemble64_world.h.  A function of the world
// through (n, row0, tile) alone: the uniform kernel and the ragged one share it, and with it every bit.  Every thread of the
// block calls it (it holds barriers).
template <int SPLIT>
__device__ __forceinline__ void ens64_world_tile(const Ensemble64Args& a, const int n, const size_t row0, const unsigned tile) {
  constexpr int TPB = kEnsembleBlock / SPLIT;  // targets per block
  extern __shared__ __attribute__((aligned(16))) unsigned char ens64_lds[];
  const Ens64WorldLds w(ens64_lds, n);
  const int hazard = ens64_stage_world(w, a.pos_in, a.weight, row0, a.fast);
  const double clamp = a.clamp;
  double px[1], py[1], ax[1], ay[1];

  if (hazard) {
    // ---- EXACT: thread = target (no barrier follows: threads without a target leave)
    if ((int)threadIdx.x >= TPB) return;
    const int t = (int)tile * TPB + (int)threadIdx.x;
    if (t >= n) return;
    const double2 p = w.spos[t];
    ens64_exact_sum(w, p.x, p.y, clamp, ax[0], ay[0]);
    ens_integrate(a, row0 + t, p.x, p.y, ax[0], ay[0]);
    return;
  }

  // ---- FAST: SPLIT consecutive lanes per target
  const int part = (int)threadIdx.x % SPLIT;
  const int t = (int)tile * TPB + (int)threadIdx.x / SPLIT;
  const bool live = t < n;
  const double2 p = w.spos[live ? t : 0];
  px[0] = p.x, py[0] = p.y;
  ens64_fast_sum<SPLIT, 1>(w, part, px, py, clamp, ax, ay);
  if (live && part == 0) ens_integrate(a, row0 + t, p.x, p.y, ax[0], ay[0]);
}

// Sweeps (nbody_sweep_*), as ensemble_kernels.hip states them: the world's entry by scalar loads once per block; a finished world
// carries its tile of pos_in over to pos_out as raw bits and returns before the staging and its barriers; otherwise delta, clamp
// and the route are the world's own in a copy of the arguments — direct_fast_f64's test on the world's clamp: FAST only with a
// clamp > 0 (a NaN fails it), for every block of the world and of its tracers.  The plain launches are the SWEEP = false
// instantiations.  No static LDS in either.
template <int SPLIT>
__device__ __forceinline__ void ens64_carry_tile(const Ensemble64Args& a, const int n, const size_t row0, const unsigned tile) {
  constexpr int TPB = kEnsembleBlock / SPLIT;
  const int t = (int)tile * TPB + (int)threadIdx.x;
  if ((int)threadIdx.x >= TPB || t >= n) return;
  const uint4* in = reinterpret_cast<const uint4*>(a.pos_in);
  uint4* out = reinterpret_cast<uint4*>(a.pos_out);
  out[row0 + t] = in[row0 + t];
}

template <int SPLIT, bool SWEEP>
__device__ __forceinline__ void ens64_step_block(const Ensemble64Args& a, const int n, const size_t row0, const unsigned tile,
                                                 const unsigned world) {
  if constexpr (SWEEP) {
    Ensemble64Args b = a;
    if (!ens64_sweep_args(b, world)) {
      ens64_carry_tile<SPLIT>(a, n, row0, tile);
      return;
    }
    ens64_world_tile<SPLIT>(b, n, row0, tile);
  } else {
    ens64_world_tile<SPLIT>(a, n, row0, tile);
  }
}

template <int SPLIT, bool SWEEP>
__global__ __launch_bounds__(kEnsembleBlock) void ensemble64_step(const Ensemble64Args a) {
  const int n = a.n_bodies;
  const unsigned world = blockIdx.x / a.tiles, tile = blockIdx.x - world * a.tiles;
  ens64_step_block<SPLIT, SWEEP>(a, n, (size_t)world * (size_t)n, tile, world);
}

// Ragged: the block's work item {row0, n | tile << 16} is the same in every lane (its address is a function of blockIdx.x
// alone, and readfirstlane says so to the compiler), so the switch on the world's lane split is taken by the whole block — the
// barriers of the staging and the butterfly of FAST see every thread.  No static LDS here either.
// Under a sweep the item's world comes from a.item_world, a table beside the items'.
template <bool SWEEP>
__global__ __launch_bounds__(kEnsembleBlock) void ensemble64_step_ragged(const Ensemble64Args a, const uint2* __restrict__ items) {
  const uint2 item = items[blockIdx.x];
  const size_t row0 = (size_t)(unsigned)__builtin_amdgcn_readfirstlane(item.x);
  const unsigned packed = __builtin_amdgcn_readfirstlane(item.y);
  const int n = (int)(packed & 0xffffu);
  const unsigned tile = packed >> 16;
  unsigned world = 0;
  if constexpr (SWEEP) world = __builtin_amdgcn_readfirstlane(a.item_world[blockIdx.x]);
  switch (ensemble_split(n)) {
    case 1: ens64_step_block<1, SWEEP>(a, n, row0, tile, world); break;
    case 2: ens64_step_block<2, SWEEP>(a, n, row0, tile, world); break;
    case 4: ens64_step_block<4, SWEEP>(a, n, row0, tile, world); break;
    case 8: ens64_step_block<8, SWEEP>(a, n, row0, tile, world); break;
    case 16: ens64_step_block<16, SWEEP>(a, n, row0, tile, world); break;
    case 32: ens64_step_block<32, SWEEP>(a, n, row0, tile, world); break;
    default: ens64_step_block<64, SWEEP>(a, n, row0, tile, world); break;
  }
}

}  // namespace

// Dynamic LDS above 64 KB (n > 3272: rows are padded to 8 and 3280 x 20 B = 65 600; the one-target-per-lane layout only) needs
// the function's limit raised: once per device and per function (`raised` is that function's own table, zero-initialised).
hipError_t ens64_raise_lds_limit(const void* kernel, std::atomic<bool>* raised) {
  int dev = 0;
  hipError_t h = hipGetDevice(&dev);
  if (h != hipSuccess) return h;
  if (dev >= 0 && dev < 64 && raised[dev]) return hipSuccess;
  h = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ensemble64_lds_bytes(kEnsembleMaxBodies));
  if (h == hipSuccess && dev >= 0 && dev < 64) raised[dev] = true;
  return h;
}

hipError_t launch_ensemble64_step(hipStream_t s, int64_t n_worlds, Ensemble64Args a) {
  if (n_worlds < 1 || a.n_bodies < 1 || a.n_bodies > kEnsembleMaxBodies || n_worlds * a.n_bodies > kEnsembleMaxRows) return hipErrorInvalidValue;
  if (a.sweep && (!a.pos_out || !a.vel)) return hipErrorInvalidValue;  // (a sweep is a step: a finished world writes pos_out)
  const int split = ensemble_split(a.n_bodies);
  const int tpb = kEnsembleBlock / split;
  a.tiles = (unsigned)((a.n_bodies + tpb - 1) / tpb);
  const dim3 grid((unsigned)(n_worlds * a.tiles));  // <= 2^26 blocks
  const size_t lds = ensemble64_lds_bytes(a.n_bodies);
  if (lds > 65536) {
    static std::atomic<bool> raised[64], raised_sweep[64];  // (each instantiation is a function of its own)
    const hipError_t h = a.sweep ? ens64_raise_lds_limit(reinterpret_cast<const void*>(&ensemble64_step<1, true>), raised_sweep)
                                 : ens64_raise_lds_limit(reinterpret_cast<const void*>(&ensemble64_step<1, false>), raised);
    if (h != hipSuccess) return h;
  }
#define NB_ENS64_GO(S)                                                                    \
  do {                                                                                  \
    if (a.sweep) {                                                                      \
      hipLaunchKernelGGL((ensemble64_step<S, true>), grid, dim3(kEnsembleBlock), lds, s, a);  \
    } else {                                                                            \
      hipLaunchKernelGGL((ensemble64_step<S, false>), grid, dim3(kEnsembleBlock), lds, s, a); \
    }                                                                                   \
  } while (0)
  switch (split) {
    case 1: NB_ENS64_GO(1); break;
    case 2: NB_ENS64_GO(2); break;
    case 4: NB_ENS64_GO(4); break;
    case 8: NB_ENS64_GO(8); break;
    case 16: NB_ENS64_GO(16); break;
    case 32: NB_ENS64_GO(32); break;
    default: NB_ENS64_GO(64); break;
  }
#undef NB_ENS64_GO
  return hipGetLastError();
}

hipError_t launch_ensemble64_step_ragged(hipStream_t s, int64_t blocks, size_t lds_bytes, const uint2* items, Ensemble64Args a) {
  if (blocks < 1 || blocks > kEnsembleMaxRows || !items || lds_bytes > ensemble64_lds_bytes(kEnsembleMaxBodies)) return hipErrorInvalidValue;
  if (a.sweep && (!a.item_world || !a.pos_out || !a.vel)) return hipErrorInvalidValue;
  if (lds_bytes > 65536) {  // its own function, so its own limit: the uniform kernel's raised one does not cover it
    static std::atomic<bool> raised[64], raised_sweep[64];
    const hipError_t h = a.sweep ? ens64_raise_lds_limit(reinterpret_cast<const void*>(&ensemble64_step_ragged<true>), raised_sweep)
                                 : ens64_raise_lds_limit(reinterpret_cast<const void*>(&ensemble64_step_ragged<false>), raised);
    if (h != hipSuccess) return h;
  }
  if (a.sweep) {
    hipLaunchKernelGGL(ensemble64_step_ragged<true>, dim3((unsigned)blocks), dim3(kEnsembleBlock), lds_bytes, s, a, items);
  } else {
    hipLaunchKernelGGL(ensemble64_step_ragged<false>, dim3((unsigned)blocks), dim3(kEnsembleBlock), lds_bytes, s, a, items);
  }
  return hipGetLastError();
}

}  // namespace nbody
