// What the f64 kernels that stage a whole world in LDS share on the device: the layout and its staging with FAST's decision
// taken on the way, the EXACT chain and the FAST sum over the staged rows.  Internal.  ensemble64_kernels.hip (the bodies of
// nbody_ensemble64_* / nbody_ragged64_* / nbody_restricted64_* / nbody_rr64_*) and, through restricted64_device.h,
// restricted64_kernels.hip and rr64_kernels.hip (the tracers of nbody_restricted64_* and nbody_rr64_*) are written over it, so
// that a pair and an order of additions are stated once: what the bodies' and the tracers' kernels promise each other bit for
// bit (restricted64_kernels.h) holds because they run this text.
//
// The FAST sum computes R targets at once from the same source reads (the bodies' kernels have R = 1).  The targets are
// independent of one another: every target has its own accumulators, and its operations and their order do not depend on R.
// The EXACT chain takes one target: its two divisions per pair are the cost, not the reads.
//
// No function here uses static LDS (ensemble64_kernels.h says why).  The including translation unit is compiled with
// -ffp-contract=off: nothing fuses unless written as an fma.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ensemble64_kernels.h"
#include "ensemble_device.h"
#include "ensemble_shape.h"
#include "fast_domain.h"
#include "pair.h"

namespace nbody {

constexpr int kEns64Run = 64;  // sources of one lane summed on their own before they join its total

// A world of n bodies in ensemble64_lds_bytes(n) of LDS: the rows padded to a multiple of kEns64TermBlock as double2 positions,
// then their u32 weights.  The pad has NaN positions and weight 0: EXACT skips its pairs (a -0.0 term), FAST never reads it.
struct Ens64WorldLds {
  double2* spos;
  uint32_t* sw;
  int n, npad;
  __device__ __forceinline__ Ens64WorldLds(unsigned char* lds, int n_bodies)
      : n(n_bodies), npad((n_bodies + kEns64TermBlock - 1) / kEns64TermBlock * kEns64TermBlock) {
    spos = reinterpret_cast<double2*>(lds);
    sw = reinterpret_cast<uint32_t*>(spos + npad);
  }
};

// The world whose rows are row0 .. row0 + n into LDS by the whole block (every thread calls it: it holds barriers) -> whether
// the world takes EXACT for this step, the same in every thread: 1 unless `fast`, and under `fast` whether one of its positions
// is outside FAST's domain.  (`fast` is uniform: every thread takes the same barriers.)
__device__ __forceinline__ int ens64_stage_world(const Ens64WorldLds& w, const double2* __restrict__ pos, const uint32_t* __restrict__ weight,
                                                 const size_t row0, const int fast) {
  int bad = 0;
  uint32_t w0 = 0;  // thread 0: the weight of source 0, whose LDS word carries the world's decision before it carries the weight
  for (int s = (int)threadIdx.x; s < w.npad; s += kEnsembleBlock) {
    double2 p = double2{__builtin_nan(""), __builtin_nan("")};
    uint32_t m = 0;
    if (s < w.n) {
      p = pos[row0 + s];
      m = weight[row0 + s];
      bad |= (int)outside_fast(p.x) | (int)outside_fast(p.y);
    }
    if (fast && s == 0) {
      w0 = m;
      m = 0;
    }
    w.spos[s] = p;
    w.sw[s] = m;
  }
  __syncthreads();
  // The block-wide OR without __syncthreads_or: its reduction takes 256 B of static LDS, and 2 x 81 920 B of dynamic LDS are
  // the CU's 160 KiB to the byte.  So sw[0] is borrowed: 0 from the staging, 1 from every wave that saw a position outside the
  // domain (the same value, whoever writes), read by all, then given its weight.
  int hazard = 1;
  if (fast) {
    if (__builtin_amdgcn_ballot_w64(bad != 0) != 0 && (threadIdx.x & 63) == 0) w.sw[0] = 1u;
    __syncthreads();
    hazard = (int)w.sw[0];
    __syncthreads();
    if (threadIdx.x == 0) w.sw[0] = w0;
    __syncthreads();
  }
  return hazard;
}

// Sweeps (nbody_sweep_*): the arguments of a block of world `world` (the same in every lane, so its entry arrives by scalar
// loads) -> false where the world has taken its steps of this call and the block has nothing to compute; otherwise delta and
// clamp become the world's own, and so does the route: direct_fast_f64's test on the world's clamp — FAST only with a clamp > 0
// (a NaN fails it).  The bodies' and the tracers' blocks of a world read the same entry and agree.
__device__ __forceinline__ bool ens64_sweep_args(Ensemble64Args& a, const unsigned world) {
  const Ens64SweepWorld sw = a.sweep[__builtin_amdgcn_readfirstlane(world)];  // (says "uniform" to the compiler)
  if (a.step >= sw.steps) return false;
  a.delta = sw.delta;
  a.clamp = sw.clamp;
  a.fast = a.fast && sw.clamp > 0.0 ? 1 : 0;
  return true;
}

// EXACT: one chain of IEEE additions for one target, from zero.  The terms of a block of kEns64TermBlock sources are evaluated
// first, branch-free (pair_term_select: the block's division chains are independent and overlap), and then added in ascending j.
__device__ __forceinline__ void ens64_exact_sum(const Ens64WorldLds& w, const double px, const double py, const double clamp, double& ax,
                                                double& ay) {
  constexpr int TB = kEns64TermBlock;
  ax = ay = 0.0;
  for (int k0 = 0; k0 < w.npad; k0 += TB) {
    double2 term[TB];
#pragma unroll
    for (int jj = 0; jj < TB; ++jj) {  // any order of evaluation ...
      const double2 q = w.spos[k0 + jj];
      term[jj] = pair_term_select(px, py, q.x, q.y, (double)w.sw[k0 + jj], clamp);
    }
#pragma unroll
    for (int jj = 0; jj < TB; ++jj) {  // ... one order of addition: ascending j
      ax = ax + term[jj].x;
      ay = ay + term[jj].y;
    }
  }
}

// FAST: the total of a target over the SPLIT consecutive lanes that share it, in every one of them.  Lane `part` takes the
// sources part, part + SPLIT, ... in ascending order, kEns64Run of them at a time (a run); within a run its 1st, 3rd, ... source
// accumulate by fma into one sum and its 2nd, 4th, ... into another, and the run ends with total = total + (the two sums added);
// the lanes' totals then meet in ens_group_sum<SPLIT>.  Every thread of the group calls it.  pair_fast(double ...) of pair.h.
template <int SPLIT, int R>
__device__ __forceinline__ void ens64_fast_sum(const Ens64WorldLds& w, const int part, const double (&px)[R], const double (&py)[R],
                                               const double clamp, double (&ax)[R], double (&ay)[R]) {
  const int cnt = (w.n - part + SPLIT - 1) / SPLIT;  // this lane's sources: part + k * SPLIT, k < cnt
#pragma unroll
  for (int r = 0; r < R; ++r) ax[r] = ay[r] = 0.0;
  for (int k0 = 0; k0 < cnt; k0 += kEns64Run) {
    const int k1 = k0 + kEns64Run < cnt ? k0 + kEns64Run : cnt;
    double x0[R], y0[R], x1[R], y1[R];
#pragma unroll
    for (int r = 0; r < R; ++r) x0[r] = y0[r] = x1[r] = y1[r] = 0.0;
    int s = part + k0 * SPLIT;
    const int s1 = part + k1 * SPLIT;
#pragma unroll 2
    for (; s + SPLIT < s1; s += 2 * SPLIT) {
      const double2 qa = w.spos[s], qb = w.spos[s + SPLIT];
      const double ma = (double)w.sw[s], mb = (double)w.sw[s + SPLIT];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        pair_fast(px[r], py[r], qa.x, qa.y, ma, clamp, x0[r], y0[r]);
        pair_fast(px[r], py[r], qb.x, qb.y, mb, clamp, x1[r], y1[r]);
      }
    }
    if (s < s1) {
      const double2 qa = w.spos[s];
      const double ma = (double)w.sw[s];
#pragma unroll
      for (int r = 0; r < R; ++r) pair_fast(px[r], py[r], qa.x, qa.y, ma, clamp, x0[r], y0[r]);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      ax[r] = ax[r] + (x0[r] + x1[r]);
      ay[r] = ay[r] + (y0[r] + y1[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    ax[r] = ens_group_sum<SPLIT>(ax[r]);
    ay[r] = ens_group_sum<SPLIT>(ay[r]);
  }
}

}  // namespace nbody
