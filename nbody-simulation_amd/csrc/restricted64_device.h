// Restricted ensembles in f64: what a block of a tracer kernel computes, stated once.  Internal, device only.
// restricted64_kernels.hip (nbody_restricted64_*: worlds x tracer tiles from the grid) and rr64_kernels.hip (nbody_rr64_*: one
// work item per block) are written over it, so that the two kernels run one text and with it share every bit, as
// restricted_tracers and rr_tracers do over rst_world_tile (restricted_device.h) in f32.  The two precisions keep two texts: a
// frame shared between them compiled to other instruction sequences.
//
// No static LDS (ensemble64_kernels.h says why).  The including translation unit is compiled with -ffp-contract=off: nothing
// fuses unless written as an fma.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nbody_hip.h"
#include "ensemble64_kernels.h"
#include "ensemble64_world.h"

namespace nbody {

// The tracer arrays of a launch, rows of all worlds together.
struct Tracer64Rows {
  double2* tpos = nullptr;      // read and (with tvel) written by their own lane only
  double2* tvel = nullptr;      // updated in place; NULL: force only, tpos is not written
  double2* tacc_out = nullptr;  // or NULL
};

// One tile of the tracers of the world whose bodies are the rows body_row0 .. body_row0 + n: the world staged in LDS with FAST's
// decision taken on the way (ens64_stage_world: the block-wide OR is the borrowed sw[0] word), the FAST sum, the EXACT arm with
// the per-tracer exception, then main.rs:419-423.  The tile's tracers are the rows tracer_row0 .. tracer_row0 + count, count <=
// kEnsembleBlock * R; lane i carries the rows tracer_row0 + i + r * 256 (coalesced), each with its own accumulators, and a lane
// past `count` computes a tracer at (0, 0) and stores nothing.  A function of the world through (body_row0, n, tracer_row0,
// count) alone.  Every thread of the block calls it (the staging holds barriers), with the same four values.  Of `b` pos_in,
// weight, delta, clamp and fast are read.
template <int R>
__device__ __forceinline__ void rst64_world_tile(const Ensemble64Args& b, const Tracer64Rows& t, const int n, const size_t body_row0,
                                                 const size_t tracer_row0, const int count) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rst64_lds[];
  const Ens64WorldLds w(rst64_lds, n);
  const int hazard = ens64_stage_world(w, b.pos_in, b.weight, body_row0, b.fast);
  const double clamp = b.clamp;

  double px[R], py[R], ax[R], ay[R];
  bool own_exact = false;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int k = (int)threadIdx.x + r * kEnsembleBlock;
    const double2 p = k < count ? t.tpos[tracer_row0 + (size_t)k] : double2{0.0, 0.0};
    px[r] = p.x, py[r] = p.y;
    own_exact |= outside_fast(p.x) || outside_fast(p.y);
  }

  // (no barrier follows the staging: the lanes may part)
  if (!hazard) ens64_fast_sum<1, R>(w, 0, px, py, clamp, ax, ay);
  if (hazard || own_exact) {  // an EXACT world: every tracer; a FAST world, rare: the tracers outside FAST's domain — one by one
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (!(hazard || outside_fast(px[r]) || outside_fast(py[r]))) continue;
      ens64_exact_sum(w, px[r], py[r], clamp, ax[r], ay[r]);
    }
  }

#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int k = (int)threadIdx.x + r * kEnsembleBlock;
    if (k >= count) continue;
    const size_t row = tracer_row0 + (size_t)k;
    if (t.tacc_out) t.tacc_out[row] = double2{ax[r], ay[r]};
    if (t.tvel) {  // main.rs:419-423, multiply then add, no contraction (TU flag)
      double2 v = t.tvel[row];
      v.x = v.x + ax[r] * b.delta;
      v.y = v.y + ay[r] * b.delta;
      const double sx = v.x * b.delta, sy = v.y * b.delta;
      t.tvel[row] = v;
      t.tpos[row] = double2{px[r] + sx, py[r] + sy};
    }
  }
}

}  // namespace nbody
