// Restricted ensembles: the tracers' step, worlds x tracer tiles in one launch (restricted_kernels.h).
//
// What every tracer computes:
//   a_t = sum_j calculate_gravity(p_t, p_j, w_j) over the bodies of its own world, j ascending      src/main.rs:234-253
//   v_t += a_t*dt ; x_t += v_t*dt                                                                   src/main.rs:419-423
// with no mass and no self term: a tracer on a body meets that body's pair like any other (EXACT's is_normal skip drops it, FAST
// adds exactly 0 through the biased denominator).
// The staging, the EXACT chain and the FAST sum are ensemble_world.h's, the text the bodies' kernel runs; a lane carries R tracers
// through them, R rows of 256 apart (coalesced), each with its own accumulators — a tracer's order of additions does not know R.
// Lanes past the end of a world's tracers compute a tracer at (0, 0) and store nothing.
//
// This translation unit is compiled with -ffp-contract=off: nothing fuses unless written as an fma.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nbody_hip.h"
#include "ensemble_world.h"
#include "restricted_kernels.h"

namespace nbody {
namespace {

template <int R>
__global__ __launch_bounds__(kEnsembleBlock) void restricted_tracers(const EnsembleArgs b, const RestrictedArgs t) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rst_lds[];
  const int n = b.n_bodies;
  const unsigned world = blockIdx.x / t.tiles, tile = blockIdx.x - world * t.tiles;
  const EnsWorldLds w(rst_lds, n);
  const int hazard = ens_stage_world(w, b.pos_in, b.mass, (size_t)world * (size_t)n, b.arith == NBODY_ARITH_AUTO);
  const float clamp = b.clamp;

  const int64_t first = (int64_t)tile * (kEnsembleBlock * R) + (int64_t)threadIdx.x;  // this lane's tracers: first + r * 256
  const size_t base = (size_t)world * (size_t)t.n_tracers;
  float px[R], py[R], ax[R], ay[R];
  bool own_exact = false;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t k = first + (int64_t)r * kEnsembleBlock;
    const float2 p = k < t.n_tracers ? t.tpos[base + (size_t)k] : make_float2(0.f, 0.f);
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
    const int64_t k = first + (int64_t)r * kEnsembleBlock;
    if (k >= t.n_tracers) continue;
    const size_t row = base + (size_t)k;
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

}  // namespace

hipError_t launch_restricted_tracers(hipStream_t s, int64_t n_worlds, const EnsembleArgs& bodies, RestrictedArgs t) {
  if (n_worlds < 1 || bodies.n_bodies < 1 || bodies.n_bodies > kEnsembleMaxBodies || n_worlds * bodies.n_bodies > kEnsembleMaxRows ||
      t.n_tracers < 1 || n_worlds > kEnsembleMaxRows / t.n_tracers || !t.tpos || !bodies.pos_in || !bodies.mass)
    return hipErrorInvalidValue;
  constexpr int64_t per_block = (int64_t)kEnsembleBlock * kRestrictedPerLane;
  t.tiles = (unsigned)((t.n_tracers + per_block - 1) / per_block);
  const dim3 grid((unsigned)(n_worlds * t.tiles));  // <= 2^26 blocks: n_worlds * n_tracers <= 2^26
  hipLaunchKernelGGL(restricted_tracers<kRestrictedPerLane>, grid, dim3(kEnsembleBlock), ensemble_lds_bytes(bodies.n_bodies), s, bodies, t);
  return hipGetLastError();
}

}  // namespace nbody
