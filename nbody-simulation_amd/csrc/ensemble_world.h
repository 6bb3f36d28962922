// What the f32 kernels that stage a whole world in LDS share on the device: the couple layout and its staging with the AUTO
// decision taken on the way, the EXACT chain and the FAST sum over the staged couples.  Internal.  ensemble_kernels.hip (the
// bodies of nbody_ensemble_* / nbody_ragged_* / nbody_restricted_*) and restricted_kernels.hip (the tracers of
// nbody_restricted_*) are written over it, so that a pair and an order of additions are stated once: what the two kernels
// promise each other bit for bit (restricted_kernels.h) holds because they run this text.
//
// Every function computes R targets at once from the same source reads (the bodies' kernel has R = 1; the tracers' kernel feeds
// 2R pairs from each couple it reads).  The targets are independent of one another: a target's operations and their order do
// not depend on R.
//
// The including translation unit is compiled with -ffp-contract=off: nothing fuses unless written as an fma.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nbody_hip.h"
#include "ensemble_kernels.h"
#include "ensemble_shape.h"
#include "fast_domain.h"
#include "pair.h"

namespace nbody {

typedef float ens_v2f __attribute__((ext_vector_type(2)));
typedef float ens_v4f __attribute__((ext_vector_type(4)));

constexpr float kEnsDenBias = 8.0779356694631609e-28f;  // 2^-90, as direct_kernels.hip
constexpr int kEnsRun = 64;                              // couples of one lane summed on their own before they join its total

// |a| + |b| as ONE v_add_f32 with abs modifiers (left to itself the compiler packs the add and pays four v_and for the moduli)
__device__ __forceinline__ float ens_abs_sum(float a, float b) {
  float r;
  asm("v_add_f32 %0, |%1|, |%2|" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// A world of n bodies in ensemble_lds_bytes(n) of LDS: (n + 1) / 2 couples {xA, xB, yA, yB}, then the masses {mA, mB} of every
// couple.  An odd n leaves the last couple's second source at (0, 0) with mass 0: FAST adds exactly 0 for it (s = 0 * rcp),
// EXACT never reads it.
struct EnsWorldLds {
  float* cplf;
  const ens_v4f* cpl;
  float* massf;
  const ens_v2f* mass2;
  int n, nc;
  __device__ __forceinline__ EnsWorldLds(unsigned char* lds, int n_bodies) : n(n_bodies), nc((n_bodies + 1) >> 1) {
    cplf = reinterpret_cast<float*>(lds);
    cpl = reinterpret_cast<const ens_v4f*>(lds);
    massf = cplf + 4 * nc;
    mass2 = reinterpret_cast<const ens_v2f*>(massf);
  }
  __device__ __forceinline__ float2 body(int t) const {
    const int o = 4 * (t >> 1) + (t & 1);
    return make_float2(cplf[o], cplf[o + 2]);
  }
};

// The world whose rows are row0 .. row0 + n into LDS by the whole block (every thread calls it: it holds a barrier) -> whether
// one of its positions is outside FAST's domain, the same in every thread — asked for with `decide`, 0 otherwise.
__device__ __forceinline__ int ens_stage_world(const EnsWorldLds& w, const float2* __restrict__ pos, const float* __restrict__ mass,
                                               const size_t row0, const bool decide) {
  int bad = 0;
  for (int s = (int)threadIdx.x; s < 2 * w.nc; s += kEnsembleBlock) {
    float2 p = make_float2(0.f, 0.f);
    float m = 0.f;
    if (s < w.n) {
      p = pos[row0 + s];
      m = mass[row0 + s];
      bad |= (int)outside_fast(p.x) | (int)outside_fast(p.y);
    }
    const int o = 4 * (s >> 1) + (s & 1);
    w.cplf[o] = p.x;
    w.cplf[o + 2] = p.y;
    w.massf[s] = m;
  }
  return __syncthreads_or(decide ? bad : 0);
}

// Sweeps (nbody_sweep_*): the arguments of a block of world `world` (the same in every lane, so its entry arrives by scalar
// loads) -> false where the world has taken its steps of this call and the block has nothing to compute; otherwise delta and
// clamp become the world's own, and so does the route: direct_arith_f32's test on the world's clamp — below kFastClampFloor, or
// NaN, the world is EXACT for the call.  The bodies' and the tracers' blocks of a world read the same entry and agree.
__device__ __forceinline__ bool ens_sweep_args(EnsembleArgs& a, const unsigned world) {
  const EnsSweepWorld sw = a.sweep[__builtin_amdgcn_readfirstlane(world)];  // (says "uniform" to the compiler)
  if (a.step >= sw.steps) return false;
  a.delta = sw.delta;
  a.clamp = sw.clamp;
  if (a.arith != NBODY_ARITH_EXACT && !(sw.clamp >= kFastClampFloor)) a.arith = NBODY_ARITH_EXACT;
  return true;
}

// EXACT: one ascending-j chain of pair_as_written<float> per target, from zero.
template <int R>
__device__ __forceinline__ void ens_exact_sum(const EnsWorldLds& w, const float (&px)[R], const float (&py)[R], const float clamp,
                                              float (&ax)[R], float (&ay)[R]) {
#pragma unroll
  for (int r = 0; r < R; ++r) ax[r] = ay[r] = 0.f;
  for (int c = 0; c < (w.n >> 1); ++c) {
    const ens_v4f s = w.cpl[c];
    const ens_v2f m = w.mass2[c];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      pair_as_written<float>(px[r], py[r], s.x, s.z, m.x, clamp, ax[r], ay[r]);
      pair_as_written<float>(px[r], py[r], s.y, s.w, m.y, clamp, ax[r], ay[r]);
    }
  }
  if (w.n & 1) {
    const ens_v4f s = w.cpl[w.nc - 1];
    const float m = w.massf[w.n - 1];
#pragma unroll
    for (int r = 0; r < R; ++r) pair_as_written<float>(px[r], py[r], s.x, s.z, m, clamp, ax[r], ay[r]);
  }
}

// FAST: the sum of lane `part` of the SPLIT lanes of a target — the couples part, part + SPLIT, ... in ascending order, the even
// and the odd sources summed apart in a packed accumulator, every run of kEnsRun couples folded (even half first) and added as
// one value to the running total.  direct_kernels.hip's pair: one v_rcp_f32, fused multiply-adds, the 2^-90 biased denominator.
template <int SPLIT, int R>
__device__ __forceinline__ void ens_fast_sum(const EnsWorldLds& w, const int part, const float (&px)[R], const float (&py)[R],
                                             const float clamp, float (&ax)[R], float (&ay)[R]) {
  const ens_v2f bias = {kEnsDenBias, kEnsDenBias};
  ens_v2f tx[R], ty[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    tx[r] = ens_v2f{px[r], px[r]};
    ty[r] = ens_v2f{py[r], py[r]};
    ax[r] = ay[r] = 0.f;
  }
  const int nc = w.nc;
  for (int c0 = part; c0 < nc; c0 += SPLIT * kEnsRun) {
    const int c1 = c0 + SPLIT * kEnsRun < nc ? c0 + SPLIT * kEnsRun : nc;
    ens_v2f accx[R], accy[R];
#pragma unroll
    for (int r = 0; r < R; ++r) accx[r] = accy[r] = ens_v2f{0.f, 0.f};
    auto couple = [&](int c) {
      const ens_v4f s = w.cpl[c];
      const ens_v2f m = w.mass2[c];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const ens_v2f dx = s.xy - tx[r], dy = s.zw - ty[r];
        ens_v2f d2 = __builtin_elementwise_fma(dy, dy, dx * dx);
        const ens_v2f sum = {ens_abs_sum(dx.x, dy.x), ens_abs_sum(dx.y, dy.y)};
        d2.x = __builtin_fmaxf(d2.x, clamp);
        d2.y = __builtin_fmaxf(d2.y, clamp);
        const ens_v2f den = __builtin_elementwise_fma(sum, d2, bias);
        const ens_v2f rc = {__builtin_amdgcn_rcpf(den.x), __builtin_amdgcn_rcpf(den.y)};
        const ens_v2f sc = m * rc;
        accx[r] = __builtin_elementwise_fma(dx, sc, accx[r]);
        accy[r] = __builtin_elementwise_fma(dy, sc, accy[r]);
      }
    };
    int c = c0;
    for (; c + 3 * SPLIT < c1; c += 4 * SPLIT) {  // (unrolled by hand: a loop with an asm statement in it is not unrolled for us)
      couple(c);
      couple(c + SPLIT);
      couple(c + 2 * SPLIT);
      couple(c + 3 * SPLIT);
    }
    for (; c < c1; c += SPLIT) couple(c);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      ax[r] = ax[r] + (accx[r].x + accx[r].y);
      ay[r] = ay[r] + (accy[r].x + accy[r].y);
    }
  }
}

}  // namespace nbody
