// Restricted ensembles in f64: the tracers' step, worlds x tracer tiles in one launch (restricted64_kernels.h).
//
// What every tracer computes, in double:
//   a_t = sum_j calculate_gravity(p_t, p_j, w_j as f64) over the bodies of its own world, j ascending      src/main.rs:234-253
//   v_t += a_t*dt ; x_t += v_t*dt                                                                          src/main.rs:419-423
// with no mass and no self term: a tracer on a body meets that body's pair like any other (EXACT's is_normal skip drops it, FAST
// adds exactly 0 through the biased denominator).
// The staging, the EXACT chain and the FAST sum are ensemble64_world.h's, the text the bodies' kernel runs; a lane carries R
// tracers through them, R rows of 256 apart (coalesced), each with its own accumulators — a tracer's order of additions does not
// know R.  Lanes past the end of a world's tracers compute a tracer at (0, 0) and store nothing.  No static LDS.
//
// This translation unit is compiled with -ffp-contract=off: nothing fuses unless written as an fma.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nbody_hip.h"
#include "ensemble64_world.h"
#include "restricted64_kernels.h"

namespace nbody {
namespace {

template <int R>
__global__ __launch_bounds__(kEnsembleBlock) void restricted64_tracers(const Ensemble64Args b, const Restricted64Args t) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rst64_lds[];
  const int n = b.n_bodies;
  const unsigned world = blockIdx.x / t.tiles, tile = blockIdx.x - world * t.tiles;
  const Ens64WorldLds w(rst64_lds, n);
  const int hazard = ens64_stage_world(w, b.pos_in, b.weight, (size_t)world * (size_t)n, b.fast);
  const double clamp = b.clamp;

  const int64_t first = (int64_t)tile * (kEnsembleBlock * R) + (int64_t)threadIdx.x;  // this lane's tracers: first + r * 256
  const size_t base = (size_t)world * (size_t)t.n_tracers;
  double px[R], py[R], ax[R], ay[R];
  bool own_exact = false;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t k = first + (int64_t)r * kEnsembleBlock;
    const double2 p = k < t.n_tracers ? t.tpos[base + (size_t)k] : double2{0.0, 0.0};
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
    const int64_t k = first + (int64_t)r * kEnsembleBlock;
    if (k >= t.n_tracers) continue;
    const size_t row = base + (size_t)k;
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

}  // namespace

hipError_t launch_restricted64_tracers(hipStream_t s, int64_t n_worlds, const Ensemble64Args& bodies, Restricted64Args t) {
  if (n_worlds < 1 || bodies.n_bodies < 1 || bodies.n_bodies > kEnsembleMaxBodies || n_worlds * bodies.n_bodies > kEnsembleMaxRows ||
      t.n_tracers < 1 || n_worlds > kEnsembleMaxRows / t.n_tracers || !t.tpos || !bodies.pos_in || !bodies.weight)
    return hipErrorInvalidValue;
  constexpr int64_t per_block = (int64_t)kEnsembleBlock * kRestricted64PerLane;
  t.tiles = (unsigned)((t.n_tracers + per_block - 1) / per_block);
  const dim3 grid((unsigned)(n_worlds * t.tiles));  // <= 2^26 blocks: n_worlds * n_tracers <= 2^26
  const size_t lds = ensemble64_lds_bytes(bodies.n_bodies);
  if (lds > 65536) {  // its own function, so its own limit: the bodies' kernels' raised ones do not cover it
    static std::atomic<bool> raised[64];
    const hipError_t h = ens64_raise_lds_limit(reinterpret_cast<const void*>(&restricted64_tracers<kRestricted64PerLane>), raised);
    if (h != hipSuccess) return h;
  }
  hipLaunchKernelGGL(restricted64_tracers<kRestricted64PerLane>, grid, dim3(kEnsembleBlock), lds, s, bodies, t);
  return hipGetLastError();
}

}  // namespace nbody
