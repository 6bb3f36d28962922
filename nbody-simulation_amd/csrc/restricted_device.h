// Restricted ensembles: what a block of a tracer kernel computes, stated once.  Internal, device only.  restricted_kernels.hip
// (nbody_restricted_*: worlds x tracer tiles from the grid) and rr_kernels.hip (nbody_rr_*: one work item per block) are written
// over it, so that the two kernels run one text and with it share every bit, as ensemble_step and ensemble_step_ragged do over
// ens_world_tile.
//
// The including translation unit is compiled with -ffp-contract=off: nothing fuses unless written as an fma.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nbody_hip.h"
#include "ensemble_kernels.h"
#include "ensemble_world.h"

namespace nbody {

// The tracer arrays of a launch, rows of all worlds together.
struct TracerRows {
  float2* tpos = nullptr;      // read and (with tvel) written by their own lane only
  float2* tvel = nullptr;      // updated in place; NULL: force only, tpos is not written
  float2* tacc_out = nullptr;  // or NULL
};

// One tile of the tracers of the world whose bodies are the rows body_row0 .. body_row0 + n: the world staged in LDS with the
// AUTO decision taken on the way, the EXACT / FAST / AUTO arms with the per-tracer exception, then main.rs:419-423.  The tile's
// tracers are the rows tracer_row0 .. tracer_row0 + count, count <= kEnsembleBlock * R; lane i carries the rows tracer_row0 + i
// + r * 256 (coalesced), each with its own accumulators, and a lane past `count` computes a tracer at (0, 0) and stores nothing.
// A function of the world through (body_row0, n, tracer_row0, count) alone.  Every thread of the block calls it (it holds a
// barrier), with the same four values.  Of `b` pos_in, mass, delta, clamp and arith are read.
template <int R>
__device__ __forceinline__ void rst_world_tile(const EnsembleArgs& b, const TracerRows& t, const int n, const size_t body_row0,
                                               const size_t tracer_row0, const int count) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rst_lds[];
  const EnsWorldLds w(rst_lds, n);
  const int hazard = ens_stage_world(w, b.pos_in, b.mass, body_row0, b.arith == NBODY_ARITH_AUTO);
  const float clamp = b.clamp;

  float px[R], py[R], ax[R], ay[R];
  bool own_exact = false;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int k = (int)threadIdx.x + r * kEnsembleBlock;
    const float2 p = k < count ? t.tpos[tracer_row0 + (size_t)k] : make_float2(0.f, 0.f);
    px[r] = p.x, py[r] = p.y;
    own_exact |= outside_fast(p.x) || outside_fast(p.y);
  }

  if (b.arith == NBODY_ARITH_EXACT || hazard) {
    ens_exact_sum<R>(w, px, py, clamp, ax, ay);
  } else {
    ens_fast_sum<1, R>(w, 0, px, py, clamp, ax, ay);
    if (b.arith == NBODY_ARITH_AUTO && own_exact) {  // rare: the tracers of this lane that are outside FAST's domain, one by one
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (!(outside_fast(px[r]) || outside_fast(py[r]))) continue;
        const float qx[1] = {px[r]}, qy[1] = {py[r]};
        float ex[1], ey[1];
        ens_exact_sum<1>(w, qx, qy, clamp, ex, ey);
        ax[r] = ex[0], ay[r] = ey[0];
      }
    }
  }

#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int k = (int)threadIdx.x + r * kEnsembleBlock;
    if (k >= count) continue;
    const size_t row = tracer_row0 + (size_t)k;
    if (t.tacc_out) t.tacc_out[row] = make_float2(ax[r], ay[r]);
    if (t.tvel) {  // main.rs:419-423, multiply then add, no contraction (TU flag)
      float2 v = t.tvel[row];
      v.x = v.x + ax[r] * b.delta;
      v.y = v.y + ay[r] * b.delta;
      const float sx = v.x * b.delta, sy = v.y * b.delta;
      t.tvel[row] = v;
      t.tpos[row] = make_float2(px[r] + sx, py[r] + sy);
    }
  }
}

}  // namespace nbody
