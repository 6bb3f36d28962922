// What is f64 about an ensemble, for the driver of ensemble_driver.h: the masses kept as the caller's u32 weights (the kernel
// converts on use, `weight as f64` is exact), the opt-in FAST rule of the f64 direct step, the kernel of ensemble64_kernels.hip.
// Internal; ensemble64.hip (nbody_ensemble64_*), ragged64.hip (nbody_ragged64_*), restricted64.hip (nbody_restricted64_*,
// which adds the tracers' launch for restricted_driver.h) and rr64.hip (nbody_rr64_*, which adds the tracers' launch over work
// items for rr_driver.h) build their handles over it.
#pragma once
#include "ensemble64_kernels.h"
#include "ensemble_driver.h"

namespace nbody {

struct EnsF64 {
  using Real = double;
  using Vec2 = double2;
  using Mass = uint32_t;
  using Args = Ensemble64Args;
  static constexpr const char* kCreate = "nbody_ensemble64_create";
  static constexpr const char* kWho = "ensemble";
  static const uint32_t* stage(const uint32_t* weight, size_t rows, std::vector<uint32_t>& tmp) {
    if (weight) return weight;  // uploaded from where they are
    tmp.assign(rows, 1u);
    return tmp.data();
  }
  static void route(Ensemble64Args& a, const uint32_t* weight, const nbody_params& p) {
    a.weight = weight;
    a.clamp = (double)p.clamp;  // the f32 parameter widened, as the f64 context's direct step does
    a.fast = direct_fast_f64(p.arith, a.clamp) ? 1 : 0;  // opt-in, and a clamp that is not > 0 (or NaN): every world EXACT
  }
  using SweepWorld = Ens64SweepWorld;
  static Ens64SweepWorld sweep_world(double delta, float clamp, int32_t steps) { return Ens64SweepWorld{delta, (double)clamp, steps, 0}; }
  static void sweep_route(Ensemble64Args& a, const nbody_params& p) { a.fast = p.arith == NBODY_ARITH_FAST ? 1 : 0; }  // (direct_fast_f64's clamp test: per world, in the kernel)
  static hipError_t launch(hipStream_t s, int64_t n_worlds, const Ensemble64Args& a) { return launch_ensemble64_step(s, n_worlds, a); }
  static hipError_t launch_resident(hipStream_t s, int64_t n_worlds, const uint2* worlds, size_t lds_bytes, const Ensemble64Args& a) {
    return launch_ensemble64_resident(s, n_worlds, worlds, lds_bytes, a);
  }
  static size_t resident_lds_bytes(int n_bodies) { return ensemble64_resident_lds_bytes(n_bodies); }
};

}  // namespace nbody
